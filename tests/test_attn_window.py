"""Sliding-window attention away from the GPU: key validation, the fp32 torch path, the programs' param."""
import pytest
import torch

from polyaxon_amd.ops import attn_window as aw


def test_key_validation():
    assert aw.KEYS == ("attn_window",) and aw.DEFAULTS == {"attn_window": 0}
    assert [aw.validate("attn_window", v) for v in (0, 1, 64.0, 2 ** 30)] == [0, 1, 64, 2 ** 30]
    st = aw.AttnWindowState("cpu", 40)
    for bad in (-1, 0.5, 2 ** 30 + 1, float("nan")):
        with pytest.raises(ValueError):
            st.set(attn_window=bad)   # through validate(); a rejected call changes nothing
    assert st.win.dtype == torch.int32 and st.win.tolist() == [40] and st.W == 40


@pytest.mark.parametrize("W", [0, 1, 5, 100])
def test_fallback_is_the_banded_softmax(W):
    from polyaxon_amd.ops.attention import flash_attention

    g = torch.Generator().manual_seed(W)
    q, k, v = (torch.randn(2, h, 19, 16, generator=g, requires_grad=True) for h in (4, 2, 2))
    out = flash_attention(q, k, v, causal=True, scale=0.5, window=aw.AttnWindowState("cpu", W))
    i, j = torch.arange(19)[:, None], torch.arange(19)[None, :]
    hidden = (j > i) | ((j <= i - W) if W > 0 else (j > i))
    kk, vv = k.repeat_interleave(2, 1), v.repeat_interleave(2, 1)
    want = (((q @ kk.transpose(-1, -2)) * 0.5).masked_fill(hidden, float("-inf")).softmax(-1) @ vv).transpose(1, 2)
    dout = torch.randn(2, 19, 4, 16, generator=g)
    assert torch.allclose(out, want, atol=1e-6)
    for a, b in zip(torch.autograd.grad(out, (q, k, v), dout), torch.autograd.grad(want, (q, k, v), dout)):
        assert torch.allclose(a, b, atol=1e-5)


def test_program_keys_and_rejections():
    from polyaxon_amd.polyflow.programs import build_program

    plain = build_program("gpt2_tiny", {}, "cpu")
    every = build_program("gpt2_tiny", {"attn_window": True, "attn_dropout": True, "dropout": True}, "cpu")
    assert every.hp_keys == plain.hp_keys + ("dropout", "attn_dropout", "attn_window")
    every.executor.set_hparams(attn_window=8)
    assert all(b.attn._window.W == 8 for b in every.executor.model.blocks)
    for name in ("resnet_tiny", "mlp"):
        with pytest.raises(ValueError, match="attn_window"):
            build_program(name, {"attn_window": True}, "cpu")
