"""The edge-tile MFMA GEMM (csrc/gemm_edge.hip via ops/gemm.py) on data whose expected output is exact.

Operand entries are integers in [-4, 4]: with K <= 4104 every partial sum stays below 16 * 4104 < 2^24, so fp32
accumulation is exact in any order (split-K included) and the only rounding is the final bf16 conversion; the outputs
must EQUAL the float64 reference rounded to bf16."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
SENTINEL = 7.0


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def _operand(x, kmajor, device):
    """x [R][K] (float64, CPU) in the asked layout: the leading slice of a buffer whose remainder is NaN, so a read
    past the operand's end poisons the result"""
    flat = (x if kmajor else x.t()).reshape(-1).to(torch.bfloat16)
    buf = torch.full((flat.numel() + 8192,), float("nan"), dtype=torch.bfloat16, device=device)
    buf[:flat.numel()] = flat.to(device)
    return buf[:flat.numel()]


@pytest.mark.parametrize("a_kmajor,b_kmajor", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(8, 8, 8), (136, 248, 72), (376, 136, 184), (128, 128, 64)])
def test_edge_layouts_shapes_exact(cuda, a_kmajor, b_kmajor, M, N, K):
    """128 x 128 x 64 tile: less than one tile in every dimension; one tile plus one 8-chunk (M, K) and two tiles less
    one chunk (N); several tiles with a tail of tile - 8; exactly one tile.  The output is a strided view inside a
    sentinel-filled buffer with guard rows: nothing outside C[M][N] may change."""
    from polyaxon_amd.ops import gemm

    assert gemm._native.lib("plx_gemm_edge").plx_gemm_edge_tile() == 128
    A, B = _ints((M, K), -4, 4, 1), _ints((N, K), -4, 4, 2)
    a, b = _operand(A, a_kmajor, cuda), _operand(B, b_kmajor, cuda)
    guard, ldc = 3, N + 16
    buf = torch.full((M + 2 * guard, ldc), SENTINEL, dtype=torch.bfloat16, device=cuda)
    out = buf[guard:guard + M, :N]
    gemm.gemm(a, b, M, N, K, a_kmajor, b_kmajor, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), (A @ B.t()).to(torch.bfloat16))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[guard:guard + M, :N] = False
    assert bool((buf[outside] == SENTINEL).all())


@pytest.mark.parametrize("epilogue", ["plain", "accumulate", "bias"])
@pytest.mark.parametrize("M,N,K", [(72, 136, 4104), (136, 72, 2056)])
def test_edge_split_k_epilogues_exact_and_reproducible(cuda, epilogue, M, N, K):
    """Weight-gradient layout (both MN-major), K split over fp32 slabs with a ragged last split; alpha = 0.5 with and
    without accumulating into an integer C, or an fp32 integer bias.  Two runs are bitwise identical."""
    from polyaxon_amd.ops import gemm

    assert gemm._native.size("plx_gemm_edge", "plx_gemm_edge_splits", M, N, K) > 1
    A, B = _ints((M, K), -4, 4, 3), _ints((N, K), -4, 4, 4)
    a, b = _operand(A, False, cuda), _operand(B, False, cuda)
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
        gemm.gemm(a, b, M, N, K, False, False, out=out, **kw)
        outs.append(out.cpu())
    assert torch.equal(outs[0], ref.to(torch.bfloat16))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("with_bias", [False, True])
def test_lm_linear_on_the_edge_kernel(cuda, monkeypatch, with_bias):
    """PLX_LM_GEMM_EDGE=1: lm.linear runs forward, data gradient and weight gradient of a non-256 shape on the kernel;
    on the integer data every GEMM output is exact, so they equal fp32 autograd of F.linear rounded to bf16."""
    from polyaxon_amd.ops import gemm, lm

    monkeypatch.setenv("PLX_LM_GEMM_EDGE", "1")
    monkeypatch.delenv("PLX_LM_GEMM", raising=False)
    gemm._seen.clear()
    X, W, DY = _ints((2, 100, 72), -4, 4, 7), _ints((136, 72), -4, 4, 8), _ints((2, 100, 136), -4, 4, 9)
    Bv = _ints((136,), -64, 64, 10)
    x = X.to(torch.bfloat16).to(cuda).requires_grad_()
    w = W.to(torch.bfloat16).to(cuda).requires_grad_()
    b = Bv.float().to(cuda).requires_grad_() if with_bias else None
    y = lm.linear(x, w, b)
    assert "Mfma" in type(y.grad_fn).__name__
    y.backward(DY.to(torch.bfloat16).to(cuda))
    xr, wr = X.float().requires_grad_(), W.float().requires_grad_()
    br = Bv.float().requires_grad_() if with_bias else None
    yr = F.linear(xr, wr, br)
    yr.backward(DY.float())
    torch.cuda.synchronize()
    for got, want in ((y, yr), (x.grad, xr.grad), (w.grad, wr.grad)):
        assert torch.equal(got.detach().cpu(), want.detach().to(torch.bfloat16))
    if with_bias:
        assert torch.equal(b.grad.cpu(), br.grad)
    d = gemm.decisions()
    for key in ("200x136x72:KK", "200x72x136:KN", "136x72x200:MN"):
        assert d[key] == {"native": True, "schedule": gemm.EDGE}
    gemm._seen.clear()
