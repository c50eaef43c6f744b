"""The "mx" FP8 recipe without a GPU (ops/fp8.py mx_*): the E8M0 scale byte rule, the `fp8_recipe` option's refusals,
and lm.linear(fp8=True, fp8_recipe="mx") on CPU tensors (the block fake-quant arithmetic)."""
import pytest
import torch
import torch.nn.functional as F

from polyaxon_amd.ops import fp8, lm


@pytest.mark.parametrize("amax,want", [(0.0, 127), (float("inf"), 127), (float("nan"), 127), (448.0, 127), (449.0, 128),
                                       (3.0, 120), (2.0 ** -133, 1)])
def test_mx_scale_byte(amax, want):
    """byte = 127 - e, 2^e = scale_for(amax).  E5M2's FMAX is 2^7 x E4M3's, so its byte is 7 lower for a finite
    positive amax -- down to the floor of 1 that scale_for's cap e <= 126 sets (the bf16 subnormal hits it in both)."""
    assert fp8.mx_scale_byte(amax, fp8.E4M3) == want
    assert fp8.mx_scale_byte(amax, fp8.E5M2) == (max(want - 7, 1) if 0 < amax < float("inf") else 127)


def test_fp8_recipe_refusals():
    from polyaxon_amd.polyflow.programs import build_program

    x, w = torch.zeros(32, 32), torch.zeros(32, 32)
    with pytest.raises(ValueError, match="fp8=True"):
        lm.linear(x, w, fp8_recipe="mx")
    with pytest.raises(ValueError, match="fp8_recipe"):
        lm.linear(x, w, fp8=True, fp8_recipe="block")
    with pytest.raises(ValueError, match="fp8: true"):
        build_program("gpt2_tiny", {"fp8_recipe": "mx"}, "cpu")
    with pytest.raises(ValueError, match="fp8_recipe"):
        build_program("gpt2_tiny", {"fp8": True, "fp8_recipe": "block"}, "cpu")
    with pytest.raises(ValueError, match="true or false"):
        build_program("gpt2_tiny", {"fp8": "mx"}, "cpu")
    with pytest.raises(ValueError, match="fp8"):
        build_program("mlp", {"fp8_recipe": "mx"}, "cpu")
    assert build_program("gpt2_tiny", {"fp8": True, "fp8_recipe": "mx"}, "cpu").info["fp8_recipe"] == "mx"


def block_ints(R, C, seed):
    """[R][C] float64: integers in [-4, 4], a 4 forced into every 32-block of every row and of every column, each
    32 x 32 square times 2^p, p in {-1, 0, 1}: every block's amax is 4 * 2^p in both directions, and E4M3 and E5M2
    hold every scaled entry exactly."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (R, C), generator=g).double()
    x[:, ::32] = 4
    x[::32, :] = 4
    p = torch.randint(-1, 2, ((R + 31) // 32, (C + 31) // 32), generator=g).double()
    return x * torch.exp2(p.repeat_interleave(32, 0).repeat_interleave(32, 1)[:R, :C])


def test_linear_mx_cpu_is_the_block_fake_quant_arithmetic():
    """Gaussian data whose 32-blocks differ in magnitude: y, dx, dW and db equal the mx_quantize_reference math
    written out, each operand blocked along the axis its GEMM contracts (dW: along tokens); the scale bytes are
    mx_scale_byte of the block maxima.  Block-integer data: they equal plain fp32 autograd of F.linear."""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(2, 32, 64, generator=g) * torch.exp2(torch.arange(64) // 32 * 5.0)).requires_grad_()
    w = (torch.randn(96, 64, generator=g) * torch.exp2(torch.arange(96) // 32 * 3.0)[:, None]).requires_grad_()
    b, dy = torch.randn(96, generator=g, requires_grad=True), torch.randn(2, 32, 96, generator=g)
    y = lm.linear(x, w, b, fp8=True, fp8_recipe="mx")
    assert type(y.grad_fn).__name__ == "_LinearMxFp8RefBackward"
    y.backward(dy)
    ref = lambda t, fmt=fp8.E4M3: fp8.mx_quantize_reference(t, fmt)[0]  # noqa: E731
    x2, w2, d2 = x.detach().view(-1, 64), w.detach(), dy.view(-1, 96)
    assert torch.equal(y.detach().view(-1, 96), ref(x2) @ ref(w2).t() + b.detach())
    assert torch.equal(x.grad.view(-1, 64), ref(d2, fp8.E5M2) @ ref(w2.t()).t())
    assert torch.equal(w.grad, ref(d2.t(), fp8.E5M2) @ ref(x2.t()).t())
    assert torch.equal(b.grad, d2.sum(0))
    assert not torch.equal(y.detach(), F.linear(x, w, b).detach())  # the quantisation is really there
    assert not torch.equal(y.detach(), lm.linear(x, w, b, fp8=True).detach())  # and it is not the per-tensor one
    vals, bytes_ = fp8.mx_quantize_reference(x2, fp8.E4M3)
    amax = x2.view(-1, 2, 32).abs().amax(-1)
    assert bytes_.tolist() == [[fp8.mx_scale_byte(float(a), fp8.E4M3) for a in row] for row in amax]

    X, W, DY = block_ints(64, 96, 1), block_ints(160, 96, 2), block_ints(64, 160, 3)
    got = [X.float().requires_grad_(), W.float().requires_grad_()]
    want = [X.float().requires_grad_(), W.float().requires_grad_()]
    lm.linear(*got, fp8=True, fp8_recipe="mx").backward(DY.float())
    F.linear(*want).backward(DY.float())
    assert torch.equal(got[0].grad, want[0].grad) and torch.equal(got[1].grad, want[1].grad)
    assert torch.equal(lm.linear(X.float(), W.float(), fp8=True, fp8_recipe="mx"), F.linear(X.float(), W.float()))
