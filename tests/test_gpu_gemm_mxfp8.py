"""The MXFP8 path (csrc/gemm_mxfp8.hip via ops/fp8.py mx_*): the one-pass cast against the block fake-quant reference
bit for bit, scale words included, and the scaled-MFMA GEMM on data whose expected output is exact.

Block-integer operands (test_mxfp8.block_ints): integers in [-4, 4] with a 4 in every 32-block of every row and
column, each 32 x 32 square times 2^p, p in {-1, 0, 1}.  A block's scale follows from its amax 4 * 2^p, so scales
differ by row, by K-block and by row-tile: a wrong lane-to-byte mapping, op_sel or word index cannot pass.  Every
product term is a multiple of 2^-2 of magnitude at most 64; over K <= 4128 every partial sum in units of 2^-2 stays
below 2^20, so fp32 accumulation is exact in any order (split-K included) and the outputs must EQUAL the float64
reference rounded to bf16."""
import pytest
import torch
import torch.nn.functional as F

from test_gemm_bounds import U, gelu64, gelu_err
from test_gpu_gemm_fp8 import F8, SENTINEL, _ints, _operand
from test_mxfp8 import block_ints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _rehome(t, fill):
    """t as the leading slice of a buffer whose remainder is `fill`"""
    buf = torch.full((t.numel() + 8192,), fill, dtype=torch.uint8, device=t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf[:t.numel()].view(t.shape)


def _quantized(x, fmt, device):
    """(q, sq) of x through the cast, q followed by 0x7f bytes (NaN in E4M3, a huge number in E5M2) and the scale
    words by 0xff bytes (NaN in E8M0): a read past either end poisons the result.  The cast takes rows in multiples of
    32, the GEMM in multiples of 16: x is cast with zero rows appended and the first len(x) rows are kept (the blocks
    of q run along K, so the extra rows change nothing)."""
    from polyaxon_amd.ops import fp8

    R = x.shape[0]
    q, sq, _, _ = fp8.mx_quantize(_operand(F.pad(x, (0, 0, 0, -R % 32)), device), fmt)
    return _rehome(q[:R], 0x7F), _rehome(sq[:, :R].contiguous(), 0xFF)


def _want_cast(x, fmt):
    """(bytes [R][C], scale words [ceil(C / 128)][R][4]) of bf16 x, blocks along C"""
    from polyaxon_amd.ops import fp8

    R, C = x.shape
    _, b = fp8.mx_quantize_reference(x, fmt)
    q = (x.float() * torch.exp2(127 - b.float()).repeat_interleave(32, 1)).to(F8[fmt]).view(torch.uint8)
    words = torch.full(((C + 127) // 128, R, 4), 127, dtype=torch.uint8)
    for kb in range(C // 32):
        words[kb // 4, :, kb % 4] = b[:, kb]
    return q, words


@pytest.mark.parametrize("fmt", [0, 1], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("R,C", [(32, 32), (96, 160), (128, 128), (160, 288)])
def test_cast_is_bit_exact(cuda, fmt, R, C):
    """Random signs, magnitudes log-uniform over 2^-10 inside a block, each 32 x 32 square times its own 2^p, p in
    [-20, 20]: neighbouring blocks need different scales in both directions.  The four outputs sit inside sentinel
    buffers; the scale words are compared whole, pad bytes included."""
    from polyaxon_amd.ops import _native

    g = torch.Generator().manual_seed(R + C + fmt)
    x = 3.0 * torch.exp2(-10 * torch.rand(R, C, generator=g)) * (1 - 2 * torch.randint(0, 2, (R, C), generator=g))
    p = torch.randint(-20, 21, (R // 32, C // 32), generator=g).float()
    x = (x * torch.exp2(p.repeat_interleave(32, 0).repeat_interleave(32, 1))).to(torch.bfloat16)
    sizes = [R * C, (C + 127) // 128 * R * 4, R * C, (R + 127) // 128 * C * 4]  # q, sq, qt, sqt
    bufs = [torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=cuda) for n in sizes]
    rc = _native.lib("plx_gemm_mxfp8").plx_mxfp8_cast(_operand(x, cuda).data_ptr(), *(b[64:].data_ptr() for b in bufs),
                                                      R, C, fmt, _native.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    want = [*_want_cast(x, fmt), *_want_cast(x.t().contiguous(), fmt)]
    for b, n, w in zip(bufs, sizes, want):
        assert torch.equal(b[64:64 + n].cpu(), w.reshape(-1))
        assert bool((b[:64] == 0xA5).all()) and bool((b[64 + n:] == 0xA5).all())


@pytest.mark.parametrize("a_fmt", [0, 1], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("M,N,K", [(16, 16, 32), (144, 240, 160), (368, 144, 288), (128, 128, 128)])
def test_gemm_exact_on_block_integers(cuda, a_fmt, M, N, K):
    """128 x 128 x 128 tile: one MX block (three of a K-tile's four lane groups multiply staged zeros); one tile plus
    one block with a scale word of one live byte; several tiles with a K tail of one block; exactly one tile.  The
    output is a strided view inside a sentinel buffer with guard rows."""
    from polyaxon_amd.ops import _native, fp8

    assert _native.lib("plx_gemm_mxfp8").plx_gemm_mxfp8_tile() == 128
    A, B = block_ints(M, K, 1), block_ints(N, K, 2)
    (a, sa), (b, sb) = _quantized(A, a_fmt, cuda), _quantized(B, 0, cuda)
    guard, ldc = 3, N + 16
    buf = torch.full((M + 2 * guard, ldc), SENTINEL, dtype=torch.bfloat16, device=cuda)
    out = buf[guard:guard + M, :N]
    fp8.mx_gemm(a, a_fmt, sa, b, sb, M, N, K, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), (A @ B.t()).to(torch.bfloat16))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[guard:guard + M, :N] = False
    assert bool((buf[outside] == SENTINEL).all())


@pytest.mark.parametrize("epilogue", ["plain", "accumulate", "bias"])
@pytest.mark.parametrize("M,N,K", [(80, 144, 4128), (144, 80, 2080)])
def test_split_k_epilogues_exact_and_reproducible(cuda, epilogue, M, N, K):
    """K split over fp32 slabs with a ragged last split; alpha = 0.5 with and without accumulating into an integer C,
    or an fp32 integer bias.  Two runs are bitwise identical."""
    from polyaxon_amd.ops import _native, fp8

    assert _native.size("plx_gemm_mxfp8", "plx_gemm_mxfp8_splits", M, N, K) > 1
    A, B = block_ints(M, K, 3), block_ints(N, K, 4)
    (a, sa), (b, sb) = _quantized(A, 1, cuda), _quantized(B, 0, cuda)
    c0, bias = _ints((M, N), -64, 64, 5), _ints((N,), -64, 64, 6)
    ref = A @ B.t()
    if epilogue == "bias":
        ref, kw = ref + bias, {"bias": bias.float().to(cuda)}
    elif epilogue == "accumulate":
        ref, kw = 0.5 * ref + c0, {"accumulate": True, "alpha": 0.5}
    else:
        ref, kw = 0.5 * ref, {"alpha": 0.5}
    outs = []
    for _ in range(2):
        out = c0.to(torch.bfloat16).to(cuda)
        fp8.mx_gemm(a, 1, sa, b, sb, M, N, K, out=out, **kw)
        outs.append(out.cpu())
    assert torch.equal(outs[0], ref.to(torch.bfloat16))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("case", ["plain", "bias", "gelu"])
def test_lm_linear_mxfp8(cuda, case):
    """lm.linear(fp8=True, fp8_recipe="mx") at 2 x 112 tokens, in 96, out 160: on block-integer data every GEMM output
    is exact, so y and the gradients equal fp32 autograd of F.linear rounded to bf16.  With the GELU epilogue h is
    exact and y is held to test_gemm_bounds.py's gelu_out bound against fp64 tanh-GELU of h."""
    from polyaxon_amd.ops import lm

    X, W, DY = block_ints(224, 96, 7).view(2, 112, 96), block_ints(160, 96, 8), block_ints(224, 160, 9).view(2, 112, 160)
    Bv = _ints((160,), -64, 64, 10)
    if case == "gelu":  # |h| of order 1 to 8, multiples of 1/256: both tails of the activation and between them
        W, Bv = W / 64, Bv / 8
    x = X.to(torch.bfloat16).to(cuda).requires_grad_()
    w = W.to(torch.bfloat16).to(cuda).requires_grad_()
    b = Bv.float().to(cuda).requires_grad_() if case != "plain" else None
    y = lm.linear(x, w, b, act="gelu_tanh" if case == "gelu" else None, fp8=True, fp8_recipe="mx")
    assert type(y.grad_fn).__name__ == "_LinearMxFp8Backward"
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert not any(t.dtype == torch.bfloat16 and t.numel() == x.numel() for t in saved)
    xr, wr = X.float().requires_grad_(), W.float().requires_grad_()
    br = Bv.float().requires_grad_() if b is not None else None
    hr = F.linear(xr, wr, br)
    if case == "gelu":
        (h,) = [t for t in saved if t.dtype == torch.bfloat16]
        torch.cuda.synchronize()
        assert torch.equal(h.cpu(), hr.detach().view(-1, 160).to(torch.bfloat16))
        h64 = h.cpu().double()
        err = (y.detach().cpu().view(-1, 160).double() - gelu64(h64)).abs()
        bound = U * gelu64(h64).abs() + (1 + U) * gelu_err(h64)
        print("gelu_out max err / bound:", float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all())
        return
    y.backward(DY.to(torch.bfloat16).to(cuda))
    hr.backward(DY.float())
    torch.cuda.synchronize()
    for got, want in ((y, hr), (x.grad, xr.grad), (w.grad, wr.grad)):
        assert torch.equal(got.detach().cpu(), want.detach().to(torch.bfloat16))
    if b is not None:
        assert torch.equal(b.grad.cpu(), br.grad)
