"""The FP8 path (csrc/gemm_fp8.hip via ops/fp8.py): the cast against torch's float8 conversion bit for bit, and the
GEMM on data whose expected output is exact.

GEMM operand entries are integers in [-4, 4] with one entry forced to 4: E4M3 and E5M2 hold them exactly under any
power-of-two scale, and with K <= 4112 every partial sum stays below 16 * 4112 < 2^24, so fp32 accumulation is exact
in any order (split-K included) and the only rounding is the final bf16 conversion; the outputs must EQUAL the float64
reference rounded to bf16."""
import pytest
import torch
import torch.nn.functional as F

from test_gemm_bounds import U, gelu64, gelu_err

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
F8 = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _ints(shape, lo, hi, seed):
    x = torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()
    x.view(-1)[seed % x.numel()] = hi  # amax is hi whatever the draw
    return x


def _operand(x, device):
    """bf16 x as the leading slice of a buffer whose remainder is NaN: a read past the end poisons the result"""
    flat = x.reshape(-1).to(torch.bfloat16)
    buf = torch.full((flat.numel() + 8192,), float("nan"), dtype=torch.bfloat16, device=device)
    buf[:flat.numel()] = flat.to(device)
    return buf[:flat.numel()].view(x.shape)


def _quantized(x, fmt, device):
    """(q, inv_scale) of integer x through the kernels, q re-homed as the leading slice of a buffer of 0x7f bytes
    (NaN in E4M3, a huge number in E5M2)"""
    from polyaxon_amd.ops import fp8

    q, _, inv = fp8.quantize(_operand(x, device), fmt)
    buf = torch.full((q.numel() + 8192,), 0x7F, dtype=torch.uint8, device=device)
    buf[:q.numel()] = q.view(-1)
    return buf[:q.numel()].view(q.shape), inv


@pytest.mark.parametrize("fmt", [0, 1], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("R,C", [(16, 16), (80, 144), (64, 64)])
def test_cast_is_bit_exact(cuda, fmt, R, C):
    """Random signs, magnitudes log-uniform in [2^-10, 1] amax: every scaled value is a normal number of the format.
    Both outputs sit inside sentinel buffers."""
    from polyaxon_amd.ops import _native, fp8

    g = torch.Generator().manual_seed(R + C + fmt)
    x = 3.0 * torch.exp2(-10 * torch.rand(R, C, generator=g)) * (1 - 2 * torch.randint(0, 2, (R, C), generator=g))
    x = x.to(torch.bfloat16)
    scale = fp8.scale_for(float(x.float().abs().max()), fmt)
    xd = _operand(x, cuda)
    words = fp8.amax_scale(xd, fmt)
    bufs = [torch.full((R * C + 128,), 0xA5, dtype=torch.uint8, device=cuda) for _ in range(2)]
    rc = _native.lib("plx_gemm_fp8").plx_fp8_cast(xd.data_ptr(), bufs[0][64:].data_ptr(), bufs[1][64:].data_ptr(), R, C,
                                                  fmt, words.data_ptr(), _native.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert words[:3].tolist() == [float(x.float().abs().max()), scale, 1 / scale]
    want = (x.float() * scale).to(F8[fmt]).view(torch.uint8)
    assert torch.equal(bufs[0][64:64 + R * C].cpu().view(R, C), want)
    assert torch.equal(bufs[1][64:64 + R * C].cpu().view(C, R), want.t())
    for b in bufs:
        assert bool((b[:64] == 0xA5).all()) and bool((b[64 + R * C:] == 0xA5).all())


@pytest.mark.parametrize("a_fmt", [0, 1], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("M,N,K", [(16, 16, 16), (144, 240, 144), (368, 144, 272), (128, 128, 128)])
def test_gemm_exact_on_integers(cuda, a_fmt, M, N, K):
    """128 x 128 x 128 tile: less than a tile everywhere; one tile plus one 16-chunk; several tiles with a tail of
    tile - 16; exactly one tile.  The output is a strided view inside a sentinel buffer with guard rows."""
    from polyaxon_amd.ops import _native, fp8

    assert _native.lib("plx_gemm_fp8").plx_gemm_fp8_tile() == 128
    A, B = _ints((M, K), -4, 4, 1), _ints((N, K), -4, 4, 2)
    (a, ia), (b, ib) = _quantized(A, a_fmt, cuda), _quantized(B, 0, cuda)
    guard, ldc = 3, N + 16
    buf = torch.full((M + 2 * guard, ldc), SENTINEL, dtype=torch.bfloat16, device=cuda)
    out = buf[guard:guard + M, :N]
    fp8.gemm(a, a_fmt, ia, b, ib, M, N, K, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), (A @ B.t()).to(torch.bfloat16))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[guard:guard + M, :N] = False
    assert bool((buf[outside] == SENTINEL).all())


@pytest.mark.parametrize("epilogue", ["plain", "accumulate", "bias"])
@pytest.mark.parametrize("M,N,K", [(80, 144, 4112), (144, 80, 2064)])
def test_split_k_epilogues_exact_and_reproducible(cuda, epilogue, M, N, K):
    """K split over fp32 slabs with a ragged last split; alpha = 0.5 with and without accumulating into an integer C,
    or an fp32 integer bias.  Two runs are bitwise identical."""
    from polyaxon_amd.ops import _native, fp8

    assert _native.size("plx_gemm_fp8", "plx_gemm_fp8_splits", M, N, K) > 1
    A, B = _ints((M, K), -4, 4, 3), _ints((N, K), -4, 4, 4)
    (a, ia), (b, ib) = _quantized(A, 1, cuda), _quantized(B, 0, cuda)
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
        fp8.gemm(a, 1, ia, b, ib, M, N, K, out=out, **kw)
        outs.append(out.cpu())
    assert torch.equal(outs[0], ref.to(torch.bfloat16))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("case", ["plain", "bias", "gelu"])
def test_lm_linear_fp8(cuda, case):
    """lm.linear(fp8=True) at 2 x 104 tokens, in 80, out 144: on the integer data every GEMM output is exact, so y and
    the gradients equal fp32 autograd of F.linear rounded to bf16.  With the GELU epilogue h is exact and y is held to
    test_gemm_bounds.py's gelu_out bound against fp64 tanh-GELU of h."""
    from polyaxon_amd.ops import lm

    X, W, DY = _ints((2, 104, 80), -4, 4, 7), _ints((144, 80), -4, 4, 8), _ints((2, 104, 144), -4, 4, 9)
    Bv = _ints((144,), -64, 64, 10)
    if case == "gelu":  # |h| of order 1 to 8, multiples of 1/64: both tails of the activation and between them
        W, Bv = W / 64, Bv / 8
    x = X.to(torch.bfloat16).to(cuda).requires_grad_()
    w = W.to(torch.bfloat16).to(cuda).requires_grad_()
    b = Bv.float().to(cuda).requires_grad_() if case != "plain" else None
    y = lm.linear(x, w, b, act="gelu_tanh" if case == "gelu" else None, fp8=True)
    assert type(y.grad_fn).__name__ == "_LinearFp8Backward"
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert not any(t.dtype == torch.bfloat16 and t.numel() == x.numel() for t in saved)
    xr, wr = X.float().requires_grad_(), W.float().requires_grad_()
    br = Bv.float().requires_grad_() if b is not None else None
    hr = F.linear(xr, wr, br)
    if case == "gelu":
        (h,) = [t for t in saved if t.dtype == torch.bfloat16]
        torch.cuda.synchronize()
        assert torch.equal(h.cpu(), hr.detach().view(-1, 144).to(torch.bfloat16))
        h64 = h.cpu().double()
        err = (y.detach().cpu().view(-1, 144).double() - gelu64(h64)).abs()
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
