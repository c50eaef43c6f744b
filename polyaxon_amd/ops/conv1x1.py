"""Stride-1 1x1 convolution on NHWC bf16 activations as three MFMA GEMMs (csrc/conv_gemm.hip).

ResNet-50's bottleneck conv1/conv3 are 33 of its 53 convolutions.  On channels_last activations each pass is
a plain GEMM over the M = N·H·W pixel rows, so instead of MIOpen's implicit-GEMM convolutions (which zero
their output with an extra SubTensorOp launch before every call and accumulate the weight gradient in a
fp32 workspace that is then cast to bf16 and added into the fp32 master gradient) the op runs:

* forward     ``y = x · Wᵀ``            — ``plx_gemm_nt`` (bf16 out)
* data grad   ``dx = dy · W``           — ``plx_gemm_nt`` against the pre-transposed bf16 ``Wᵀ``
* weight grad ``dW = dyᵀ · x``           — ``plx_gemm_tn`` split over M, accumulated in fp32 directly

The fp32 master weight is cast to bf16 (and transposed) once per forward by ``plx_weight_prep``; the weight
gradient comes back in fp32, so autocast's bf16 weight copy and its backward cast disappear too.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from polyaxon_amd.ops import _native, side_stream, wcache
from polyaxon_amd.ops.flat import direct_grad

_CUS: Dict[int, int] = {}

# A/B knob, read once at load: 1 = a BatchNorm backward hands its dx pass to the data-gradient GEMM of the 1x1
# convolution that produced its input (DxSink, plx_gemm_nt_bndx); 0 = the dx pass and the GEMM as two kernels
_BN_DX_FUSED = os.environ.get("PLX_BN_DX_FUSED", "1") != "0"


def set_bn_dx_fused(on: bool) -> bool:
    """Switch the fused BatchNorm-dx data gradient for the graphs built from now on; returns the previous setting."""
    global _BN_DX_FUSED
    prev, _BN_DX_FUSED = _BN_DX_FUSED, bool(on)
    return prev


# A/B knob, read once at load: 1 = a bottleneck's last BatchNorm leaves its apply + residual + ReLU pass to the forward
# GEMM of the next block's conv1 (PendingApply, plx_gemm_nt_bnapply); 0 = the apply pass and the GEMM as two kernels
_BN_APPLY_FUSED = os.environ.get("PLX_BN_APPLY_FUSED", "1") != "0"


def set_bn_apply_fused(on: bool) -> bool:
    """Switch the fused BatchNorm-apply forward GEMM for the forwards run from now on; returns the previous setting."""
    global _BN_APPLY_FUSED
    prev, _BN_APPLY_FUSED = _BN_APPLY_FUSED, bool(on)
    return prev


def bn_apply_fused() -> bool:
    return _BN_APPLY_FUSED


# A/B knob, read once at load: 1 = where a BatchNorm-dx data gradient (DxSink) belongs to a convolution with Cin = 64 and
# Cout <= 256 whose weight gradient accumulates into its flat slot with atomics, one kernel forms both gradients and the
# BatchNorm's dx is never stored (plx_gemm_nt_bndx_wgrad); 0 = plx_gemm_nt_bndx and the side stream's plx_gemm_tn
_DGRAD_WGRAD_FUSED = os.environ.get("PLX_DGRAD_WGRAD_FUSED", "1") != "0"


def set_dgrad_wgrad_fused(on: bool) -> bool:
    """Switch the fused data + weight gradient for the backwards run from now on; returns the previous setting."""
    global _DGRAD_WGRAD_FUSED
    prev, _DGRAD_WGRAD_FUSED = _DGRAD_WGRAD_FUSED, bool(on)
    return prev


def dgrad_wgrad_fused_ok(cin: int, cout: int) -> bool:
    """The shape class and mode of the fused data + weight gradient: one 64-wide N tile, at most four K stages (the dW
    accumulators live in registers), and the atomic weight-gradient mode (the kernel has no deterministic reduction)."""
    return (_DGRAD_WGRAD_FUSED and cin == 64 and cout <= 256 and cout % 64 == 0
            and bool(_native.lib("plx_conv").plx_get_tn_atomic()))


# A/B knob, read once at load: a downsampling block's bn3 backward no longer writes d_residual = dy * mask3 -- the
# downsample BatchNorm's backward takes (dy, mask3) instead (BnLink.foreign).  1 = route A (:func:`ds_bwd_route`) where
# conv3's data gradient also forms its weight gradient (layer 1.0), route B elsewhere; 2 = route A wherever conv3 has a
# dx sink (layer 2.0 too); 0 = the dx pass writes d_residual and the downsample BatchNorm reads it back
_DS_BWD_FUSED = int(os.environ.get("PLX_DS_BWD_FUSED", "1") or 0)


def set_ds_bwd_fused(mode: int) -> int:
    """Set the downsampling blocks' backward mode (0, 1 or 2) for the backwards run from now on; returns the previous."""
    global _DS_BWD_FUSED
    prev, _DS_BWD_FUSED = _DS_BWD_FUSED, int(mode)
    return prev


def ds_bwd_route(cin: int, cout: int, has_sink: bool, mode: int = None, wgrad_fused: bool = None) -> str:
    """How the backward of a downsampling block's bn3 (``cout`` channels, behind conv3 with ``cin`` inputs) hands the
    residual's gradient to the downsample BatchNorm.

    * ``"A"``: bn3 runs its reduce / finalize only; conv3's data-gradient GEMM forms bn3's dx (``has_sink``: conv3
      attached a :class:`DxSink`, and the next block's conv1 reduced bn3's partials, so bn3 has no pass of its own
      left), and the downsample BatchNorm runs its own reduce on (dy, mask3).  Taken where that
      GEMM also forms conv3's weight gradient (``wgrad_fused``, default :func:`dgrad_wgrad_fused_ok`: layer 1.0 with
      atomic weight gradients), so neither dx nor d_residual is stored; with mode 2 wherever conv3 has a sink.
    * ``"B"``: bn3's dx pass stays and reduces the downsample BatchNorm's partials (ResBn) but writes no d_residual;
      the downsample BatchNorm's dx reads (dy, mask3).
    * ``"off"``: d_residual is written and read back -- mode 0, and above 2048 channels, where ``plx_bn_backward``
      refuses a ResBn."""
    mode = _DS_BWD_FUSED if mode is None else mode
    if not mode or cout > 2048:
        return "off"
    if has_sink and mode >= 2:
        return "A"
    if has_sink and (dgrad_wgrad_fused_ok(cin, cout) if wgrad_fused is None else wgrad_fused):
        return "A"
    return "B"


def _num_cus(dev: torch.device) -> int:
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _CUS:
        _CUS[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _CUS[idx]


def _stream() -> int:
    return _native.current_stream()


def nt_stats_rows(n: int) -> int:
    """Rows per block of plx_gemm_nt for an N-wide output (the granularity of its BN-stats partials)."""
    return _native.size("plx_conv", "plx_gemm_nt_rows_per_block", n)


def _check_stats(stats, m: int, n: int) -> None:
    """``stats`` (or None) can hold the channel-stats partials of an M x N output, fp32 [2][nblk][N]."""
    if stats is not None:
        nblk = -(-m // nt_stats_rows(n))
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= 2 * nblk * n


def _check_add(add, add_mask, m: int, n: int) -> None:
    """``add`` (or None) is a bf16 [M][N] epilogue addend; ``add_mask`` (or None) its 1-bit mask over dense rows."""
    if add is not None:
        assert add.shape == (m, n) and add.stride(1) == 1 and add.dtype == torch.bfloat16 and add.data_ptr() % 16 == 0
    if add_mask is not None:
        assert add is not None and add.stride(0) == n and add_mask.dtype == torch.uint8 and add_mask.numel() == m * n // 8


def gemm_nt(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor = None, stats: torch.Tensor = None,
            add: torch.Tensor = None, bnr: "_native.GemmBnBwdArgs" = None,
            add_mask: torch.Tensor = None) -> torch.Tensor:
    """out[M][N] = a[M][K] · b[N][K]ᵀ, bf16 (rows may be strided, K contiguous).  ``stats`` (fp32
    [2][ceil(M / nt_stats_rows(N))][N]) receives per-block channel sums and sums of squares of ``out``;
    ``add`` (bf16 [M][N]) is summed into the product in the epilogue, only where ``add_mask`` (a ReLU's 1-bit
    forward mask, uint8 [M*N/8]) is set when given; ``bnr`` (from :meth:`BnLink.request`) makes the epilogue
    emit the BatchNorm-backward partials of ``out``."""
    m, k = a.shape
    n = b.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=a.device)
    assert a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1 and b.shape[1] == k
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    _check_stats(stats, m, n)
    _check_add(add, add_mask, m, n)
    rc = _native.lib("plx_conv").plx_gemm_nt(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, a.stride(0),
                                             b.stride(0), out.stride(0),
                                             stats.data_ptr() if stats is not None else None,
                                             add.data_ptr() if add is not None else None,
                                             add.stride(0) if add is not None else 0,
                                             add_mask.data_ptr() if add_mask is not None else None,
                                             ctypes.addressof(bnr) if bnr is not None else None, _stream())
    _native.check(rc, "plx_gemm_nt")
    return out


def gemm_nt_bndx(g: torch.Tensor, x: torch.Tensor, mask: torch.Tensor, coef: torch.Tensor, dy: torch.Tensor,
                 b: torch.Tensor, out: torch.Tensor = None, add: torch.Tensor = None,
                 bnr: "_native.GemmBnBwdArgs" = None, add_mask: torch.Tensor = None) -> torch.Tensor:
    """The data gradient ``out[M][N] = dy · bᵀ`` of a 1x1 convolution whose incoming gradient ``dy[M][K]`` is a
    BatchNorm backward's dx, produced by the GEMM itself: ``dy = coef[0]·(g·mask) + coef[1]·x + coef[2]`` per
    channel, rounded to bf16 once (bit-identical to the standalone dx pass), written to ``dy`` and consumed as the
    GEMM's A operand.  ``g``, ``x``, ``dy``: dense bf16 rows; ``mask``: the BatchNorm's 1-bit ReLU mask or None;
    ``coef``: fp32 [3·K] from the BatchNorm backward's finalize; ``add`` / ``add_mask`` / ``bnr`` as
    :func:`gemm_nt`."""
    m, k = g.shape
    n = b.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=g.device)
    for t in (g, x, dy):
        assert t.shape == (m, k) and t.dtype == torch.bfloat16 and t.stride() == (k, 1) and t.data_ptr() % 16 == 0
    assert b.stride(1) == 1 and out.stride(1) == 1 and b.shape[1] == k and b.dtype == torch.bfloat16
    assert b.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.numel() == 3 * k
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.numel() == m * k // 8
    _check_add(add, add_mask, m, n)
    rc = _native.lib("plx_conv").plx_gemm_nt_bndx(g.data_ptr(), x.data_ptr(),
                                                  mask.data_ptr() if mask is not None else None, coef.data_ptr(),
                                                  dy.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, b.stride(0),
                                                  out.stride(0), add.data_ptr() if add is not None else None,
                                                  add.stride(0) if add is not None else 0,
                                                  add_mask.data_ptr() if add_mask is not None else None,
                                                  ctypes.addressof(bnr) if bnr is not None else None, _stream())
    _native.check(rc, "plx_gemm_nt_bndx")
    return out


def gemm_nt_bndx_wgrad(g: torch.Tensor, x: torch.Tensor, mask: torch.Tensor, coef: torch.Tensor, dy: torch.Tensor,
                       b: torch.Tensor, x_in: torch.Tensor, dw: torch.Tensor, out: torch.Tensor = None,
                       add: torch.Tensor = None, bnr: "_native.GemmBnBwdArgs" = None, add_mask: torch.Tensor = None,
                       blocks: int = 0) -> torch.Tensor:
    """:func:`gemm_nt_bndx` that also adds the convolution's weight gradient ``dw[K][N] += dyᵀ · x_in`` (fp32, float
    atomics) from the ``dy`` tiles it produces, and never stores ``dy`` (accepted, left untouched).  ``x_in``: the
    convolution's saved input, dense bf16 ``[M][N]``; N = 64 and K ≤ 256 only.  ``out`` and the ``bnr`` partials are
    bit-identical to :func:`gemm_nt_bndx`'s.  ``blocks``: 0 = one persistent block per CU; a test hook otherwise."""
    m, k = g.shape
    n = b.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=g.device)
    for t in (g, x, dy):
        assert t.shape == (m, k) and t.dtype == torch.bfloat16 and t.stride() == (k, 1) and t.data_ptr() % 16 == 0
    assert b.stride(1) == 1 and out.stride(1) == 1 and b.shape[1] == k and b.dtype == torch.bfloat16
    assert b.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.numel() == 3 * k
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.numel() == m * k // 8
    assert x_in.shape == (m, n) and x_in.dtype == torch.bfloat16 and x_in.stride() == (n, 1) and x_in.data_ptr() % 16 == 0
    assert dw.shape == (k, n) and dw.dtype == torch.float32 and dw.stride(1) == 1
    _check_add(add, add_mask, m, n)
    rc = _native.lib("plx_conv").plx_gemm_nt_bndx_wgrad(g.data_ptr(), x.data_ptr(),
                                                        mask.data_ptr() if mask is not None else None,
                                                        coef.data_ptr(), dy.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                        m, n, k, b.stride(0), out.stride(0),
                                                        add.data_ptr() if add is not None else None,
                                                        add.stride(0) if add is not None else 0,
                                                        add_mask.data_ptr() if add_mask is not None else None,
                                                        ctypes.addressof(bnr) if bnr is not None else None,
                                                        x_in.data_ptr(), dw.data_ptr(), dw.stride(0), blocks, _stream())
    _native.check(rc, "plx_gemm_nt_bndx_wgrad")
    return out


def gemm_nt_bnapply(x: torch.Tensor, res: torch.Tensor, sb: torch.Tensor, rsb, out_a: torch.Tensor, mask: torch.Tensor,
                    b: torch.Tensor, out: torch.Tensor = None, stats: torch.Tensor = None) -> torch.Tensor:
    """The forward ``out[M][N] = out_a · bᵀ`` of a 1x1 convolution whose input ``out_a[M][K]`` is the output of the
    bottleneck before it, produced by the GEMM itself: ``out_a = relu(x·sb[0] + sb[1] + (res·rsb[0] + rsb[1]))`` per
    channel (``res`` as is without ``rsb``), rounded to bf16 once, written to ``out_a`` with its sign bits to ``mask``
    (both bit-identical to the standalone apply pass) and consumed as the GEMM's A operand.  ``x``, ``res``,
    ``out_a``: dense bf16 rows; ``mask``: uint8 [M·K/8]; ``sb``, ``rsb`` (or None): fp32 [2·K]; ``stats`` as
    :func:`gemm_nt`."""
    m, k = x.shape
    n = b.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=x.device)
    for t in (x, res, out_a):
        assert t.shape == (m, k) and t.dtype == torch.bfloat16 and t.stride() == (k, 1) and t.data_ptr() % 16 == 0
    assert b.stride(1) == 1 and out.stride(1) == 1 and b.shape[1] == k and b.dtype == torch.bfloat16
    assert b.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() >= m * k // 8
    for c in (sb, rsb):
        assert c is None or (c.dtype == torch.float32 and c.is_contiguous() and c.numel() == 2 * k
                             and c.data_ptr() % 16 == 0)
    assert sb is not None
    _check_stats(stats, m, n)
    rc = _native.lib("plx_conv").plx_gemm_nt_bnapply(x.data_ptr(), res.data_ptr(), sb.data_ptr(),
                                                     rsb.data_ptr() if rsb is not None else None, out_a.data_ptr(),
                                                     mask.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k,
                                                     b.stride(0), out.stride(0),
                                                     stats.data_ptr() if stats is not None else None, _stream())
    _native.check(rc, "plx_gemm_nt_bnapply")
    return out


def gemm_tn(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor = None, accumulate: bool = False) -> torch.Tensor:
    """out[N1][N2] (fp32) = a[M][N1]ᵀ · b[M][N2]  (``+=`` with ``accumulate``)."""
    m, n1 = a.shape
    n2 = b.shape[1]
    if out is None:
        out = torch.empty(n1, n2, dtype=torch.float32, device=a.device)
        accumulate = False
    assert a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1 and b.shape[0] == m
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    lib = _native.lib("plx_conv")
    cus = _num_cus(a.device)
    ws = torch.empty(_native.size("plx_conv", "plx_gemm_tn_workspace", m, n1, n2, cus), dtype=torch.float32,
                     device=a.device)
    rc = lib.plx_gemm_tn(a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), m, n1, n2, a.stride(0),
                         b.stride(0), out.stride(0), cus, int(accumulate), _stream())
    _native.check(rc, "plx_gemm_tn")
    return out


def weight_prep(w: torch.Tensor):
    """fp32 [Cout][Cin] -> (bf16 W, bf16 Wᵀ)."""
    cout, cin = w.shape[0], w.shape[1]
    wb = torch.empty(cout, cin, dtype=torch.bfloat16, device=w.device)
    wt = torch.empty(cin, cout, dtype=torch.bfloat16, device=w.device)
    w32 = w.reshape(cout, cin)
    if w32.dtype != torch.float32 or not w32.is_contiguous():
        w32 = w32.float().contiguous()
    rc = _native.lib("plx_conv").plx_weight_prep(w32.data_ptr(), wb.data_ptr(), wt.data_ptr(), cout, cin, _stream())
    _native.check(rc, "plx_weight_prep")
    return wb, wt


class GradMailbox:
    """Hands a gradient from a later op's backward to an earlier op's backward that consumes the same tensor.

    In a ResNet identity block the block input feeds conv1 and the residual add of bn3; autograd would sum the
    two gradients with a separate bf16 add over the whole activation.  Instead bn3's backward ``put``s its
    residual gradient here and conv1's backward adds it in its data-gradient GEMM epilogue.  In a downsampling
    block the input feeds the downsample conv and conv1: conv1's backward ``put``s its data gradient and the
    downsample conv's dgrad adds it (in place, for the strided 1x1 whose GEMM only reaches the even pixels).
    The consumer runs first in the forward and ``arm``s the box only on the native path that will drain it;
    the producer defers only into an armed box and sets ``expect``.  Reverse-topological backward order (higher
    autograd sequence number first) runs the producer's backward before the consumer's; ``take`` fails loudly
    if that ever does not hold instead of silently dropping a gradient."""

    __slots__ = ("armed", "grad", "mask", "expect", "s2k1")

    def __init__(self):
        self.armed = False
        self.grad = None
        self.mask = None
        self.expect = False
        self.s2k1 = False  # the consumer is a stride-2 1x1 conv (its dgrad adds to the even-even pixels only)

    def put(self, g: torch.Tensor) -> None:
        if self.grad is not None:
            g = self._dense() + g
        self.grad, self.mask = g, None

    def put_masked(self, g: torch.Tensor, mask: torch.Tensor) -> None:
        """The gradient is ``g`` where the 1-bit ReLU ``mask`` (uint8, bit k of byte i = element 8i+k of the NHWC
        rows) is set, else 0: bn3's backward hands over its incoming gradient and forward mask instead of writing
        d_residual, and the consumer's dgrad epilogue applies the mask (``gemm_nt(add_mask=...)``)."""
        if self.grad is not None:
            self.put(unpack_relu_mask(g, mask))
            return
        self.grad, self.mask = g, mask

    def _dense(self) -> torch.Tensor:
        return self.grad if self.mask is None else unpack_relu_mask(self.grad, self.mask)

    def take(self):
        """(gradient, mask or None)."""
        g, m = self.grad, self.mask
        self.grad = self.mask = None
        if g is None and self.expect:
            raise RuntimeError("GradMailbox: the deferred gradient did not arrive before its consumer's backward")
        return g, m


def unpack_relu_mask(g: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """g * mask with the 1-bit mask expanded (channels_last NHWC element order)."""
    bits = (mask.view(-1, 1) >> torch.arange(8, device=mask.device, dtype=torch.uint8)) & 1
    n, c, h, w = g.shape
    keep = bits.view(n, h, w, c).permute(0, 3, 1, 2).to(g.dtype)
    return (g * keep).contiguous(memory_format=torch.channels_last)


class DxSink:
    """A 1x1 convolution's output → the fused BatchNorm that consumes it, for the backward: the BatchNorm hands its
    dx pass to the convolution's data-gradient GEMM (:func:`gemm_nt_bndx`).

    The convolution attaches one to its output (``y._plx_dx_sink``) when its data gradient is wide in K and narrow in
    N (:func:`dx_sink_for`: the GEMM is bound by reading the gradient, which it can as well produce).  A BatchNorm backward
    that only has dx to write (no d_residual tensor) runs its reduce / finalize, ``put``s what the dx pass would have
    read and returns the *unwritten* dx buffer as its input gradient; the convolution's backward ``take``s the
    payload, checks that the gradient it was handed is that very buffer, and its GEMM fills it on the way.  The
    payload keeps the operands alive until then."""

    __slots__ = ("payload", "cin", "cout")

    def __init__(self, cin: int = 0, cout: int = 0):
        self.payload = None
        self.cin, self.cout = cin, cout  # the convolution's channel counts (ds_bwd_route asks)

    def put(self, g: torch.Tensor, x: torch.Tensor, mask, coef: torch.Tensor, dx: torch.Tensor) -> None:
        self.payload = (g, x, mask, coef, dx)

    def take(self):
        p, self.payload = self.payload, None
        return p


def dx_sink_for(x: torch.Tensor, weight: torch.Tensor):
    """The shape-class rule of the fused BatchNorm-dx data gradient: the conv input needs a gradient, the GEMM's
    K (= Cout) is at least twice its N (= Cin), and N fits one tile (N <= 128).  With two or four N tiles per row
    panel every tile's block repeats the loads and the transform; measured alone that ties (N = 256) or loses
    (N = 512) against the two kernels (profiles/bn_dx_fused.md), so those stay on them."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return None
    cout, cin = weight.shape[0], weight.shape[1]
    return DxSink(cin, cout) if dx_sink_shape_ok(cin, cout) else None


def dx_sink_shape_ok(cin: int, cout: int) -> bool:
    """:func:`dx_sink_for`'s rule on the channel counts alone."""
    return _BN_DX_FUSED and cout >= 2 * cin and cin <= 128


class PendingApply:
    """A bottleneck's last BatchNorm → the 1x1 convolution that reads the block output, for the forward: the
    BatchNorm leaves its apply + residual + ReLU pass to the convolution's forward GEMM (:func:`gemm_nt_bnapply`).

    The BatchNorm (``ops.bn_fused.bn_act(defer_res_relu=True)``) runs its reduce / finalize only and returns the
    *unwritten* output carrying one of these (``out._plx_pending``) with what the apply pass would have read: the raw
    input ``x``, the residual ``res``, ``sb`` (fp32 [scale | bias]), ``rsb`` (the residual's deferred affine or None)
    and the ``mask`` buffer.  The model only asks for this when the next op is a supported native 1x1 convolution
    (``models.resnet``), which ``take``s the payload and whose GEMM fills ``out`` and ``mask`` on the way; any other
    consumer goes through :meth:`fill` (``ops.bn_fused.materialize``), the standalone apply kernel.  Nothing may read
    ``out`` or ``mask`` before either happened: a second ``take`` raises, and so does the BatchNorm's backward when
    the payload is still pending (:meth:`check_done`).  The payload keeps the operands alive."""

    __slots__ = ("x", "res", "sb", "rsb", "mask", "out", "state")

    def __init__(self, x, res, sb, rsb, mask, out):
        self.x, self.res, self.sb, self.rsb, self.mask, self.out = x, res, sb, rsb, mask, out
        self.state = "pending"  # -> "taken" (a GEMM fills it) or "filled" (the standalone pass did)

    @property
    def pending(self) -> bool:
        return self.state == "pending"

    def take(self) -> "PendingApply":
        if self.state != "pending":
            raise RuntimeError("PendingApply: the deferred BatchNorm output was already " + self.state
                               + "; a second consumer cannot take it")
        self.state = "taken"
        return self

    def fill(self) -> None:
        """The standalone apply + residual + ReLU pass into ``out`` and ``mask`` (no-op once done)."""
        if self.state != "pending":
            return
        n, c, h, w = self.x.shape
        rc = _native.lib("plx_bn").plx_bn_apply_res_relu(
            self.x.data_ptr(), self.res.data_ptr(), self.out.data_ptr(), n * h * w, c, self.sb.data_ptr(),
            self.mask.data_ptr(), self.rsb.data_ptr() if self.rsb is not None else None, _stream())
        _native.check(rc, "plx_bn_apply_res_relu")
        self.state = "filled"
        self.release()

    def release(self) -> None:  # the operands, and the references that make a cycle with the output tensor
        self.x = self.res = self.sb = self.rsb = self.mask = self.out = None

    def check_done(self) -> None:
        if self.state == "pending":
            raise RuntimeError("PendingApply: the BatchNorm's deferred output (and its ReLU mask) was never filled: "
                               "no consumer took it and nothing materialised it before the backward")


def fill_pending(t):
    """``t`` with a still pending deferred apply (:class:`PendingApply`) filled by the standalone kernel."""
    p = getattr(t, "_plx_pending", None) if t is not None else None
    if p is not None:
        p.fill()
    return t


def bn_apply_sink_ok(cin: int, cout: int) -> bool:
    """The shape-class rule of the fused BatchNorm-apply forward GEMM, :func:`dx_sink_for`'s mirrored: the GEMM's K
    (= Cin) is at least twice its N (= Cout), and N fits one tile (N <= 128)."""
    return _BN_APPLY_FUSED and cin >= 2 * cout and cout <= 128


class BnLink:
    """A fused BatchNorm(+ReLU)'s output → the convolution whose data gradient is that output's COMPLETE gradient.

    The BatchNorm forward attaches one to its output (``y._plx_bn_link``) holding what its backward reduction
    reads (x, ReLU mask, mean, invstd).  A consumer conv that the model marks as the sole gradient source
    (``bn_link=True``) ``request``s a partials buffer and its dgrad GEMM epilogue writes the per-block
    Σdz and Σdz·x̂ (csrc/conv_gemm.hip ``BnBwd``); the BatchNorm backward then skips its reduce pass."""

    __slots__ = ("x", "mask", "mean", "invstd", "part", "nblk", "_args", "affine", "split", "foreign")

    def __init__(self, x=None, mask=None, mean=None, invstd=None):
        self.x, self.mask, self.mean, self.invstd = x, mask, mean, invstd
        # (dy, mask3): the gradient this BatchNorm's backward receives is bn3's incoming dy as is, and its dz is
        # dy * mask3, the ReLU mask of bn3 downstream (a downsampling block with PLX_DS_BWD_FUSED: no d_residual)
        self.foreign = None
        self.affine = None  # deferred apply: fp32 [scale | bias] the consumer applies to the raw x
        self.part = None
        self.nblk = 0
        self._args = None
        self.split = 0  # > 0: the first of two GEMMs wrote rows [0, split); the strided 1x1 dgrad still owes the rest

    def _args_for(self, nblk_total: int, blk_off: int) -> "_native.GemmBnBwdArgs":
        return _native.GemmBnBwdArgs(self.x.data_ptr(), self.mask.data_ptr() if self.mask is not None else None,
                                     self.mean.data_ptr(), self.invstd.data_ptr(), self.part.data_ptr(), nblk_total,
                                     blk_off)

    def request(self, nblk: int) -> "_native.GemmBnBwdArgs":
        c = self.x.shape[1]
        self.part = torch.empty(2 * nblk * c, dtype=torch.float32, device=self.x.device)
        self.nblk, self.split = nblk, 0
        self._args = self._args_for(nblk, 0)
        return self._args

    def request_split(self, nblk1: int, nblk2: int) -> "_native.GemmBnBwdArgs":
        """ResNet downsampling block: x feeds conv1 (stride-1 1x1, dgrad deferred into the box) and the stride-2 1x1
        downsample conv (dgrad adds the box's gradient at the even-even pixels).  conv1's dgrad epilogue reduces
        the pixels the strided one never touches (rows [0, nblk1), even-even pixels skipped), and the strided
        dgrad the even-even ones with their final value (rows from nblk1, :meth:`request_rest`)."""
        n, c, h, w = self.x.shape
        self.part = torch.empty(2 * (nblk1 + nblk2) * c, dtype=torch.float32, device=self.x.device)
        self.nblk, self.split = nblk1 + nblk2, nblk1
        a = self._args_for(nblk1 + nblk2, 0)
        a.skip_h, a.skip_w = h, w
        self._args = a
        return a

    def request_rest(self) -> "_native.GemmBnBwdArgs":
        a = self._args_for(self.nblk, self.split)
        self.split = 0
        self._args = a
        return a

    def take(self):
        part, nblk = self.part, self.nblk
        if self.split:  # the second GEMM never ran: the rows are incomplete, the BatchNorm reduces itself
            part, nblk = None, 0
        self.part, self._args, self.split = None, None, 0
        return part, nblk


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[N,C,H,W] channels_last -> [N*H*W, C] view."""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c)


def bn_link_of(x: torch.Tensor, want: bool):
    link = getattr(x, "_plx_bn_link", None) if want else None
    return link if (link is not None and link.x is not None and link.x.shape == x.shape) else None


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stats, box, sink, link, dxsink=None, pend=None):
        if pend is not None and (x.data_ptr() != pend.out.data_ptr() or x.shape != pend.out.shape
                                 or x.dtype != torch.bfloat16
                                 or not x.is_contiguous(memory_format=torch.channels_last)):
            raise RuntimeError("PendingApply: the convolution's input is not the deferred BatchNorm output")
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        ctx.box = box
        ctx.dxsink = dxsink
        ctx.sink = sink if (sink is not None and sink.armed) else None
        if ctx.sink is not None:
            ctx.sink.expect = True
        # a sink nobody drains (its consumer is not on the native path) means x has another gradient source that
        # autograd adds: dx is then never x's whole gradient, so the link must not be served
        ctx.link = link if (sink is None or sink.armed) else None
        ctx.wgrad = direct_grad(weight)
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        wb, wt = wcache.lookup(weight) or weight_prep(weight)
        y = torch.empty((n, cout, h, w), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
        if pend is not None:  # fills x (the block output before this conv) and its mask, and reads x as the A operand
            gemm_nt_bnapply(_rows(pend.x), _rows(pend.res), pend.sb, pend.rsb, _rows(x), pend.mask, wb, _rows(y), stats)
            pend.release()
        else:
            gemm_nt(_rows(x), wb, _rows(y), stats)
        ctx.save_for_backward(x, wt)
        ctx.wshape = weight.shape
        ctx.wdtype = weight.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        n, cin, h, w = x.shape
        # the BatchNorm that consumed the output deferred its dx pass to this backward's data-gradient GEMM: the
        # gradient handed over must be its still unwritten dx buffer (a hook or a second consumer of the output
        # would have replaced it by a tensor computed from uninitialised memory)
        fused = ctx.dxsink.take() if ctx.dxsink is not None else None
        if fused is not None and (dy.data_ptr() != fused[4].data_ptr() or dy.shape != fused[4].shape
                                  or dy.dtype != torch.bfloat16 or not ctx.needs_input_grad[0]):
            raise RuntimeError("DxSink: the BatchNorm's deferred input gradient was replaced before the convolution's "
                               "backward could fill it")
        dy = dy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dx = dw = None
        wgrad_done = False
        extra, extra_mask = ctx.box.take() if ctx.box is not None else (None, None)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x, memory_format=torch.channels_last)
            if extra is not None and (extra.dtype != torch.bfloat16
                                      or not extra.is_contiguous(memory_format=torch.channels_last)):
                if extra_mask is not None:
                    extra, extra_mask = unpack_relu_mask(extra, extra_mask), None
                extra = extra.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            bnr = None
            # the link is only served when dx (+ the box's gradient) is the whole gradient of x: with a box, the
            # producer must actually have deferred into it; a sink means dx is only part of it -- except where the
            # sink's consumer is a strided 1x1, which only adds to the even-even pixels (BnLink.request_split)
            rows = nt_stats_rows(cin)
            if ctx.link is not None and ctx.sink is None and (ctx.box is None or extra is not None):
                bnr = ctx.link.request(-(-(n * h * w) // rows))
            elif ctx.link is not None and ctx.sink is not None and ctx.sink.s2k1 and extra is None:
                bnr = ctx.link.request_split(-(-(n * h * w) // rows), -(-(n * ((h + 1) // 2) * ((w + 1) // 2)) // rows))
            cout = ctx.wshape[0]
            if (fused is not None and ctx.needs_input_grad[1] and ctx.wgrad is not None
                    and dgrad_wgrad_fused_ok(cin, cout)):
                # one kernel on this stream forms dx and adds dW into the flat slot from the BatchNorm's dx tiles, which
                # are never stored: no weight-gradient launch follows
                g, bx, bmask, coef, _ = fused
                gemm_nt_bndx_wgrad(_rows(g), _rows(bx), bmask, coef, _rows(dy), wt, _rows(x),
                                   ctx.wgrad.as_strided((cout, cin), (cin, 1)), _rows(dx),
                                   add=_rows(extra) if extra is not None else None, bnr=bnr, add_mask=extra_mask)
                wgrad_done = True
            elif fused is not None:  # fills dy (the BatchNorm's dx) and reads it as the A operand
                g, bx, bmask, coef, _ = fused
                gemm_nt_bndx(_rows(g), _rows(bx), bmask, coef, _rows(dy), wt, _rows(dx),
                             add=_rows(extra) if extra is not None else None, bnr=bnr, add_mask=extra_mask)
            else:
                gemm_nt(_rows(dy), wt, _rows(dx), add=_rows(extra) if extra is not None else None, bnr=bnr,
                        add_mask=extra_mask)
            if ctx.sink is not None:  # the downsample conv's dgrad adds this gradient in its epilogue
                ctx.sink.put(dx)
                dx = None
        if ctx.needs_input_grad[1] and not wgrad_done:
            cout = ctx.wshape[0]
            if ctx.wgrad is not None:  # accumulate into the flat gradient slot, autograd sees no weight grad
                slot = ctx.wgrad.as_strided((cout, cin), (cin, 1))
                side_stream.run(lambda: gemm_tn(_rows(dy), _rows(x), out=slot, accumulate=True), (dy, x), x.device)
            else:
                dw = gemm_tn(_rows(dy), _rows(x)).view(ctx.wshape).to(ctx.wdtype)
        return dx, dw, None, None, None, None, None, None


def _bf16_context(x: torch.Tensor) -> bool:
    """bf16 activations, or fp32 ones inside a bf16 autocast region (an fp32 network keeps fp32 convs)."""
    if x.dtype == torch.bfloat16:
        return True
    return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16


def supported(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    return (x.is_cuda and x.dim() == 4 and _bf16_context(x) and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and conv.bias is None
            and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0 and x.numel() > 0)


def conv1x1(x: torch.Tensor, weight: torch.Tensor, with_stats: bool = False,
            grad_box: "GradMailbox" = None, grad_sink: "GradMailbox" = None, bn_link: bool = False) -> torch.Tensor:
    """With ``with_stats`` the output carries ``_plx_channel_stats`` = (fp32 [2][nblk][Cout] per-block channel
    sums / sums of squares, nblk), which a following fused BatchNorm uses instead of its own stats pass.
    ``grad_box``: add the box's deferred gradient into dx; ``grad_sink``: defer dx into that (armed) box;
    ``bn_link``: dx (+ ``grad_box``'s gradient) is the complete gradient of ``x`` — serve the BatchNorm that
    produced ``x`` its backward partials (:class:`BnLink`)."""
    stats = None
    if with_stats:
        n, _, h, w = x.shape
        m, cout = n * h * w, weight.shape[0]
        nblk = -(-m // nt_stats_rows(cout))
        stats = torch.empty(2 * nblk * cout, dtype=torch.float32, device=x.device)
    if grad_box is not None:
        grad_box.armed = True
    dxsink = dx_sink_for(x, weight)
    # the block output whose apply + residual + ReLU was left to this conv (PendingApply): taken when the shape class is
    # the fused GEMM's, else filled by the standalone pass
    pend = getattr(x, "_plx_pending", None)
    if pend is not None and pend.pending:
        n, cin, h, w = x.shape
        if bn_apply_sink_ok(cin, weight.shape[0]) and n * h * w * cin < (1 << 30):
            pend = pend.take()
        else:
            pend.fill()
            pend = None
    else:
        pend = None
    y = _Conv1x1.apply(x, weight, stats, grad_box, grad_sink, bn_link_of(x, bn_link), dxsink, pend)
    if stats is not None:
        y._plx_channel_stats = (stats, nblk)
    if dxsink is not None:
        y._plx_dx_sink = dxsink
    return y


class Conv1x1(nn.Conv2d):
    """``nn.Conv2d(in, out, 1, bias=False)`` whose GPU path is the MFMA GEMM op above (same parameter, same
    init; falls back to ``F.conv2d`` on CPU or for unsupported channel counts)."""

    def __init__(self, in_ch: int, out_ch: int, stride: int = 1, native: bool = True, bn_stats: bool = True):
        super().__init__(in_ch, out_ch, 1, stride=stride, bias=False)
        self.native = native
        self.bn_stats = bn_stats  # emit channel stats for the BatchNorm that follows (training only)

    def forward(self, x: torch.Tensor, grad_box: GradMailbox = None, grad_sink: GradMailbox = None,
                bn_link: bool = False) -> torch.Tensor:
        if self.native and supported(x, self):
            return conv1x1(x, self.weight, with_stats=self.bn_stats and self.training, grad_box=grad_box,
                           grad_sink=grad_sink, bn_link=bn_link)
        return F.conv2d(fill_pending(x), self.weight, None, self.stride)
