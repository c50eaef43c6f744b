"""ops/fp8.py without a GPU: the host twin of the kernels' scale rule, the `fp8` program param, and
lm.linear(fp8=True) on CPU tensors (the torch fake-quant arithmetic)."""
import pytest
import torch
import torch.nn.functional as F

from polyaxon_amd.ops import fp8, lm


@pytest.mark.parametrize("amax,want", [(0.0, 1.0), (float("inf"), 1.0), (float("nan"), 1.0), (448.0, 1.0),
                                       (449.0, 0.5), (1e-30, 2.0 ** 108), (3.0, 128.0)])
def test_scale_for(amax, want):
    assert fp8.scale_for(amax, fp8.E4M3) == want
    # E5M2's FMAX is 128 x E4M3's
    assert fp8.scale_for(amax, fp8.E5M2) == (want * 128 if 0 < amax < float("inf") else 1.0)


@pytest.mark.parametrize("program", ["resnet50", "mlp"])
def test_fp8_refused_outside_gpt2(program):
    from polyaxon_amd.polyflow.programs import build_program

    with pytest.raises(ValueError, match="fp8"):
        build_program(program, {"fp8": True}, "cpu")
    with pytest.raises(ValueError, match="true or false"):
        build_program("gpt2_tiny", {"fp8": 1}, "cpu")


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def test_linear_fp8_cpu_is_the_fake_quant_arithmetic():
    """Gaussian data: y, dx, dW and db equal the quantize_reference math written out; integer data (exact in both
    formats): they equal plain fp32 autograd of F.linear."""
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(2, 24, 32, generator=g, requires_grad=True), torch.randn(48, 32, generator=g, requires_grad=True)
    b, dy = torch.randn(48, generator=g, requires_grad=True), torch.randn(2, 24, 48, generator=g)
    y = lm.linear(x, w, b, fp8=True)
    assert type(y.grad_fn).__name__ == "_LinearFp8RefBackward"
    y.backward(dy)
    (xq, ix), (wq, iw) = fp8.quantize_reference(x.view(-1, 32), fp8.E4M3), fp8.quantize_reference(w, fp8.E4M3)
    dq, idy = fp8.quantize_reference(dy.view(-1, 48), fp8.E5M2)
    assert torch.equal(y.detach().view(-1, 48), (xq @ wq.t()) * (ix * iw) + b.detach())
    assert torch.equal(x.grad.view(-1, 32), (dq @ wq) * (idy * iw))
    assert torch.equal(w.grad, (dq.t() @ xq) * (idy * ix))
    assert torch.equal(b.grad, dy.view(-1, 48).sum(0))
    assert not torch.equal(y.detach(), F.linear(x, w, b).detach())  # the quantisation is really there

    X, W, DY = _ints((2, 24, 32), -4, 4, 1), _ints((48, 32), -4, 4, 2), _ints((2, 24, 48), -4, 4, 3)
    got = [X.clone().requires_grad_(), W.clone().requires_grad_()]
    ref = [X.clone().requires_grad_(), W.clone().requires_grad_()]
    lm.linear(*got, fp8=True).backward(DY)
    F.linear(*ref).backward(DY)
    assert torch.equal(got[0].grad, ref[0].grad) and torch.equal(got[1].grad, ref[1].grad)
    assert torch.equal(lm.linear(X, W, fp8=True), F.linear(X, W))
