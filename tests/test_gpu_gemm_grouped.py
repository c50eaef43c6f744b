"""The grouped MFMA GEMM (csrc/gemm_grouped.hip via ops/gemm.py, ops/moe.py) on data whose expected output is exact.

Operand entries are integers in [-4, 4]: every partial sum stays below 16 * 393 < 2^24, so fp32 accumulation is exact
and the only rounding is the final bf16 conversion; the outputs must EQUAL the float64 per-segment reference rounded
to bf16.  Operands are NaN-padded past their end and outputs sit in sentinel buffers with guard rows."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
COUNTS = [0, 1, 130, 125]  # an empty segment, one row, a tile + 2, a tile - 3; starts that are no multiple of 8


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _ints(shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def _operand(x, device):
    """x (float64, CPU) as bf16 on the device: the leading slice of a buffer whose remainder is NaN, so a read past
    the operand's end poisons the result"""
    buf = torch.full((x.numel() + 8192,), float("nan"), dtype=torch.bfloat16, device=device)
    buf[:x.numel()] = x.reshape(-1).to(torch.bfloat16).to(device)
    return buf[:x.numel()].view(x.shape)


def _offs(counts):
    return torch.tensor([0] + counts, dtype=torch.int32).cumsum(0).to(torch.int32)


def _segments(counts):
    o = _offs(counts).tolist()
    return [slice(o[e], o[e + 1]) for e in range(len(counts))]


@pytest.mark.parametrize("b_kmajor", [True, False])
@pytest.mark.parametrize("N,K", [(128, 64), (136, 72)])
def test_rows_mode_exact_and_follows_the_device_table(cuda, b_kmajor, N, K):
    """Two count vectors written into the SAME device offs tensor between two otherwise identical calls: the second
    launch follows the new table, so the sizes are device data."""
    from polyaxon_amd.ops import gemm

    assert gemm._native.lib("plx_gemm_grouped").plx_gemm_grouped_tile() == 128
    P, E, guard, ldc = 256, 4, 3, N + 16
    A, W = _ints((P, K), 1), _ints((E, N, K), 2)
    a, b = _operand(A, cuda), _operand(W if b_kmajor else W.transpose(1, 2).contiguous(), cuda)
    offs = torch.zeros(E + 1, dtype=torch.int32, device=cuda)
    for counts in (COUNTS, [256, 0, 0, 0]):
        offs.copy_(_offs(counts))
        buf = torch.full((P + 2 * guard, ldc), SENTINEL, dtype=torch.bfloat16, device=cuda)
        out = buf[guard:guard + P, :N]
        gemm.grouped_rows(a, b, offs, N, K, b_kmajor, out=out)
        ref = torch.cat([A[s] @ W[e].t() for e, s in enumerate(_segments(counts))])
        assert torch.equal(out.cpu(), ref.to(torch.bfloat16))
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[guard:guard + P, :N] = False
        assert bool((buf[outside] == SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reduce_mode_exact_empty_expert_zero_and_reproducible(cuda, dtype):
    from polyaxon_amd.ops import gemm

    counts, M, N = [0, 1, 63, 64, 65, 200], 136, 72
    P, E = sum(counts), len(counts)
    A, B = _ints((P, M), 3), _ints((P, N), 4)
    a, b, offs = _operand(A, cuda), _operand(B, cuda), _offs(counts).to(cuda)
    ref = torch.stack([A[s].t() @ B[s] for s in _segments(counts)]).to(dtype)
    outs = []
    for _ in range(2):
        buf = torch.full((E + 2, M, N), SENTINEL, dtype=dtype, device=cuda)
        gemm.grouped_wgrad(a, b, offs, E, out=buf[1:E + 1])
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[E + 1] == SENTINEL).all())
        outs.append(buf[1:E + 1].cpu())
    assert torch.equal(outs[0], ref)
    assert bool((outs[0][0] == 0).all())
    assert torch.equal(outs[0], outs[1])


def test_shape_check_refuses_without_launching(cuda):
    from polyaxon_amd.ops import gemm

    assert gemm.grouped_supported(256, 4, 136, 72)
    assert not gemm.grouped_supported(256, 4, 132, 72) and not gemm.grouped_supported(256, 4, 136, 68)
    assert not gemm.grouped_supported(256, 65, 136, 72) and not gemm.grouped_supported(1 << 22, 4, 8, 512)
    a, b = torch.zeros(264, 72, dtype=torch.bfloat16, device=cuda), torch.zeros(4, 136, 72, dtype=torch.bfloat16,
                                                                                device=cuda)
    with pytest.raises(RuntimeError, match="-1"):  # a misaligned operand
        gemm.grouped_rows(a.view(-1)[4:4 + 256 * 72].view(256, 72), b, _offs(COUNTS).to(cuda), 136, 72, True)


def test_grouped_linear_autograd_exact(cuda):
    """forward, dx and dW equal fp32 autograd of per-segment F.linear rounded to bf16"""
    from polyaxon_amd.ops import moe

    E, K, N, P = 4, 72, 136, sum(COUNTS)
    X, W, DY = _ints((P, K), 5), _ints((E, N, K), 6), _ints((P, N), 7)
    x, w = (t.to(torch.bfloat16).to(cuda).requires_grad_() for t in (X, W))
    y = moe.grouped_linear(x, w, _offs(COUNTS).to(cuda))
    assert "GroupedLinear" in type(y.grad_fn).__name__
    y.backward(DY.to(torch.bfloat16).to(cuda))
    xr, wr = X.float().requires_grad_(), W.float().requires_grad_()
    yr = torch.cat([F.linear(xr[s], wr[e]) for e, s in enumerate(_segments(COUNTS))])
    yr.backward(DY.float())
    for got, want in ((y, yr), (x.grad, xr.grad), (w.grad, wr.grad)):
        assert torch.equal(got.detach().cpu(), want.detach().to(torch.bfloat16))


@pytest.mark.parametrize("act", ["swiglu", "gelu"])
def test_experts_match_the_reference_path(cuda, act):
    """the bf16 GPU path against the fp32 reference path with the same routing: forward, dx, d-weights, d-gates, to
    the tolerance tests/test_gpu_models.py holds the fused model paths to"""
    from polyaxon_amd.ops import moe

    T, d, ff, E, k = 96, 64, 128, 4, 2
    g = torch.Generator().manual_seed(8)
    x = torch.randn(T, d, generator=g)
    up = torch.randn(E, 2 * ff if act == "swiglu" else ff, d, generator=g) / d ** 0.5
    down = torch.randn(E, d, ff, generator=g) / ff ** 0.5
    ids, gates, _ = moe.route(x, torch.randn(E, d, generator=g), k)
    dy = torch.randn(T, d, generator=g)
    res = {}
    for name, dt in (("native", torch.bfloat16), ("ref", torch.float32)):
        # the same bf16-rounded values on both paths
        leaves = [t.to(torch.bfloat16).to(dt).to(cuda).requires_grad_() for t in (x, up, down)]
        gt = gates.to(cuda).requires_grad_()
        y = moe.experts(leaves[0], ids.to(cuda), gt, leaves[1], leaves[2], act)
        assert ("Combine" in type(y.grad_fn).__name__) == (name == "native")
        y.backward(dy.to(dt).to(cuda))
        res[name] = [y.detach()] + [t.grad for t in leaves + [gt]]
    for got, want in zip(res["native"], res["ref"]):
        torch.testing.assert_close(got.float(), want.float(), rtol=3e-2, atol=3e-2 * float(want.abs().max()))


def test_captured_step_follows_the_router(cuda):
    """forward + backward of a MoE tiny Llama under torch.cuda.graph: the replay with a second token batch, which
    routes differently, gives the loss of the eager step on that batch"""
    from polyaxon_amd.models.transformer import Transformer, lm_loss, tiny_llama

    torch.manual_seed(0)
    model = Transformer(tiny_llama(n_experts=4)).to(cuda)
    batches = torch.randint(0, 256, (2, 2, 64), generator=torch.Generator().manual_seed(9)).to(cuda)
    tokens = batches[0].clone()

    def step():
        for p in model.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = lm_loss(model(tokens), tokens) + 0.01 * model.moe_aux()
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    replays = []
    for b in (1, 0, 1):
        tokens.copy_(batches[b])
        graph.replay()
        replays.append(captured.clone())
    eager = step()  # tokens hold batch 1
    assert float(replays[0]) != float(replays[1])
    torch.testing.assert_close(replays[0], eager, rtol=3e-2, atol=3e-2 * float(eager.abs()))
    assert torch.equal(replays[0], replays[2])
