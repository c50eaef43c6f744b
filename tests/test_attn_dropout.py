"""Attention dropout (ops/attn_dropout.py) without a GPU: names and validation, the state's words, the host twin of the
mask, the fp32 fallback of flash_attention against an explicit masked softmax, and the way up through the model, the
executor, the programs and the trainer.  The kernels are tested in tests/test_gpu_attn_dropout.py."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. names, validation, the state
def test_keys_threshold_scale_validate():
    from polyaxon_amd.ops import attn_dropout as ad

    assert ad.KEYS == ("attn_dropout",) and ad.DEFAULTS == {"attn_dropout": 0.0}
    assert [ad.threshold(p) for p in (0.0, 0.1, 0.5, 0.999, 0.9999)] == [0, 26, 128, 255, 255]
    assert ad.scale(0) == 1.0                                   # exactly: rate 0 is bitwise the plain attention
    for T in (1, 26, 128, 255):
        want = struct.unpack("<f", struct.pack("<f", 256.0 / (256 - T)))[0]
        assert ad.scale(T) == want and abs(ad.scale(T) * (256 - T) / 256 - 1) < 2.0 ** -23
    assert ad.scale(128) == 2.0 and ad.scale(255) == 256.0
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ad.validate("attn_dropout", bad)
    with pytest.raises(KeyError):
        ad.validate("dropout", 0.1)
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            ad.scale(bad)
    assert ad.stream_word(0, 0) == 0x80000000 and ad.stream_word(3, 5) == 0x80030005
    assert ad.stream_word(32767, 65535) == 0xFFFFFFFF
    for layer, bh in ((32768, 0), (0, 65536), (-1, 0)):
        with pytest.raises(ValueError):
            ad.stream_word(layer, bh)


def test_state_words_and_whole_call_rejection():
    from polyaxon_amd.ops import attn_dropout as ad
    from polyaxon_amd.ops.dropout import key_words

    step = torch.zeros(1, dtype=torch.int32)
    st = ad.AttnDropoutState("cpu", step, seed=(7 << 32) | 9, rank=0)
    assert st.hp.dtype == torch.int32 and st.hp.numel() == 4
    assert st.words() == (0, 0x3F800000, 9, 7) and st.hp.tolist() == [0, 0x3F800000, 9, 7]
    st.set(attn_dropout=0.5)
    assert st.T == 128 and st.c == 2.0 and st.hp.tolist() == [128, 0x40000000, 9, 7]
    with pytest.raises(ValueError):
        st.set(attn_dropout=1.0)
    with pytest.raises(KeyError):
        st.set(attn_dropout=0.1, dropout=0.1)
    assert st.host == {"attn_dropout": 0.5} and st.hp.tolist()[0] == 128   # a rejected call changes nothing
    st.set_rank(3)
    assert st.key == key_words((7 << 32) | 9, 3) == (9, 7 ^ 3) and st.hp.tolist()[2:] == [9, 4]
    step += 5
    assert st.step() == 5


def test_module_is_torch_free():
    code = ("import sys; import polyaxon_amd.ops.attn_dropout as m; import polyaxon_amd.polyflow.programs; "
            "assert m.threshold(0.1) == 26; assert m.mask_reference((1, 2), 0, 0, 0, 5, 7, 26).shape == (5, 7); "
            "assert 'torch' not in sys.modules, 'torch was imported'")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ------------------------------------------------------------------ 2. the twin
KEY = (0x1234ABCD, 0x0F0F1E1E)


def test_twin_is_the_contract_element_by_element():
    """The vectorised twin against the contract spelled out one element at a time."""
    from polyaxon_amd.ops import attn_dropout as ad
    from polyaxon_amd.polytune.sampler import philox4x32_10

    step, layer, bh, T = 11, 3, 70, 128
    m = ad.mask_reference(KEY, step, layer, bh, 13, 22, T)
    assert m.shape == (13, 22) and m.dtype == np.bool_
    for q in range(13):
        for k in range(22):
            w = philox4x32_10([q >> 2], [k >> 2], [step], [0x80000000 | (layer << 16) | bh], *KEY)
            byte = (int(w[q & 3][0]) >> (8 * (k & 3))) & 0xFF
            assert bool(m[q, k]) == (byte >= T), (q, k)


@pytest.mark.parametrize("T", [26, 128, 255])
def test_twin_kept_count(T):
    """The kept count of a 257 x 257 mask within 5 binomial sigma of n (1 - T / 256), for the keys the GPU tests use."""
    from polyaxon_amd.ops import attn_dropout as ad

    n, p = 257 * 257, T / 256.0
    for key, step, layer, bh in ((KEY, 3, 1, 0), (KEY, 4, 0, 5), ((5, 0), 0, 0, 0)):
        kept = int(ad.mask_reference(key, step, layer, bh, 257, 257, T).sum())
        z = abs(kept - n * (1 - p)) / math.sqrt(n * p * (1 - p))
        print(f"T={T} key={key} step={step} layer={layer} bh={bh}: kept {kept} z={z:.2f}")
        assert z <= 5.0


def test_twin_properties():
    from polyaxon_amd.ops import attn_dropout as ad

    assert ad.mask_reference(KEY, 3, 1, 0, 257, 257, 0).all()          # T = 0 keeps everything
    base = ad.mask_reference(KEY, 3, 1, 0, 257, 257, 128)
    for other in (ad.mask_reference(KEY, 4, 1, 0, 257, 257, 128), ad.mask_reference(KEY, 3, 2, 0, 257, 257, 128),
                  ad.mask_reference(KEY, 3, 1, 1, 257, 257, 128), ad.mask_reference((KEY[0] + 1, KEY[1]), 3, 1, 0,
                                                                                    257, 257, 128)):
        agree = float((other == base).mean())
        assert 0.45 < agree < 0.55, agree                              # independent masks of rate 1/2 agree on half
    # a monotone family: what a higher threshold keeps, a lower one keeps too
    assert not (ad.mask_reference(KEY, 3, 1, 0, 257, 257, 255) & ~base).any()
    # tiling independence: the mask of a sub-range is the slice of the full mask, on and off the 4 x 4 block grid
    for q0, k0, nq, nk in ((0, 0, 100, 31), (32, 64, 32, 64), (33, 65, 30, 50), (255, 3, 2, 254), (128, 256, 129, 1)):
        assert np.array_equal(ad.mask_reference(KEY, 3, 1, 0, nq, nk, 128, q0=q0, k0=k0),
                              base[q0:q0 + nq, k0:k0 + nk]), (q0, k0)


# ------------------------------------------------------------------ 3. the fp32 fallback
def _explicit(q, k, v, causal, scale, keep, c):
    """softmax, then the mask, spelled out per (batch, head) with GQA by indexing."""
    B, H, S, D = q.shape
    G = H // k.shape[1]
    out = []
    for b in range(B):
        for h in range(H):
            s = (q[b, h] @ k[b, h // G].T) * scale
            if causal:
                s = s.masked_fill(torch.ones_like(s, dtype=torch.bool).triu(1), -math.inf)
            p = torch.softmax(s, -1) * keep[b * H + h] * c
            out.append(p @ v[b, h // G])
    return torch.stack(out).view(B, H, S, D).transpose(1, 2)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [0, 26, 128, 255])
def test_fallback_is_the_masked_softmax(T, causal):
    from polyaxon_amd.ops import attn_dropout as ad
    from polyaxon_amd.ops.attention import flash_attention

    B, H, Hkv, S, Skv, D, layer = 2, 4, 2, 9, 13, 16, 2
    gen = torch.Generator().manual_seed(T + causal)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_()  # noqa: E731
    q, k, v = mk(B, H, S, D), mk(B, Hkv, Skv, D), mk(B, Hkv, Skv, D)
    g = torch.randn(B, S, H, D, generator=gen, dtype=torch.float64)
    st = ad.AttnDropoutState("cpu", torch.full((1,), 6, dtype=torch.int32), seed=KEY[0] | (KEY[1] << 32))
    st.set(attn_dropout=T / 256.0)
    assert st.T == T
    keep = torch.from_numpy(np.stack([ad.mask_reference(st.key, 6, layer, bh, S, Skv, T) for bh in range(B * H)]))
    got = flash_attention(q, k, v, causal=causal, scale=0.3, drop=(st, layer))
    grads = torch.autograd.grad(got, (q, k, v), g)
    q2, k2, v2 = (t.detach().clone().requires_grad_() for t in (q, k, v))
    want = _explicit(q2, k2, v2, causal, 0.3, keep.double(), st.c)
    wgrads = torch.autograd.grad(want, (q2, k2, v2), g)
    # the fallback computes in fp32
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
    for a, b in zip(grads, wgrads):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
    if T == 0:
        assert torch.equal(got, flash_attention(q, k, v, causal=causal, scale=0.3))
    else:
        assert not torch.equal(got, flash_attention(q, k, v, causal=causal, scale=0.3))
        st.step_counter += 1        # another step, another mask
        assert not torch.equal(got, flash_attention(q, k, v, causal=causal, scale=0.3, drop=(st, layer)))


# ------------------------------------------------------------------ 4. model
def _tiny(**kw):
    from polyaxon_amd.models.transformer import Transformer, gpt2_125m

    torch.manual_seed(0)
    return Transformer(gpt2_125m(vocab_size=64, n_layers=2, d_model=32, n_heads=2, d_ff=64, max_seq_len=16, **kw))


def test_model_train_only_and_layers(monkeypatch):
    from polyaxon_amd.ops import attn_dropout as ad

    model = _tiny()
    tokens = torch.randint(0, 64, (2, 16))
    model.train()
    plain = model(tokens)
    st = ad.AttnDropoutState("cpu", torch.zeros(1, dtype=torch.int32), seed=1)
    st.set(attn_dropout=0.5)
    model.set_attn_dropout(st)
    assert [blk.attn._drop for blk in model.blocks] == [(st, 0), (st, 1)]
    seen = []
    real = ad.mask_reference
    monkeypatch.setattr(ad, "mask_reference", lambda key, step, layer, bh, *a: (seen.append((layer, bh)),
                                                                                 real(key, step, layer, bh, *a))[1])
    assert not torch.equal(model(tokens), plain)
    assert set(seen) == {(l, bh) for l in range(2) for bh in range(4)}   # every layer, every b * H + h
    model.eval()
    monkeypatch.setattr(ad, "mask_reference", lambda *a, **k: pytest.fail("a mask was drawn in eval()"))
    assert torch.equal(model(tokens), plain)
    model.train()
    model.set_attn_dropout(None)
    assert torch.equal(model(tokens), plain)


def test_checkpointed_blocks_redraw_the_same_masks():
    from polyaxon_amd.models.transformer import lm_loss
    from polyaxon_amd.ops import attn_dropout as ad

    a, b = _tiny(), _tiny(checkpoint=True)
    b.load_state_dict(a.state_dict())
    tokens = torch.randint(0, 64, (2, 16))
    st = ad.AttnDropoutState("cpu", torch.zeros(1, dtype=torch.int32), seed=2)
    st.set(attn_dropout=0.4)
    grads = []
    for m in (a, b):
        m.train()
        m.set_attn_dropout(st)
        loss = lm_loss(m(tokens), tokens)
        loss.backward()
        grads.append((loss.detach(), m.blocks[0].attn.qkv.weight.grad.clone()))
    torch.testing.assert_close(grads[0][0], grads[1][0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(grads[0][1], grads[1][1], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------ 5. executor, programs, example, trainer
def _run(params, seed, steps, **hp):
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("gpt2_tiny", params, "cpu")
    ex = prog.executor
    ex.reset(seed=seed)
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k not in ("dropout", "attn_dropout")}
    ex.set_hparams(**base, **hp)
    ex.run(steps)
    return prog, ex


def test_executor_routes_attn_dropout():
    _, plain = _run({}, 4, 3, attn_dropout=0.5)  # without the param the key is dropped
    assert plain.attn_dropout is None and plain.dropout is None
    _, zero = _run({"attn_dropout": True}, 4, 3, attn_dropout=0.0)
    assert zero.dropout is None and zero.attn_dropout.step_counter is zero.step
    assert torch.equal(zero.flat.params, plain.flat.params) and torch.equal(zero.losses(), plain.losses())
    _, half = _run({"attn_dropout": True}, 4, 3, attn_dropout=0.5)
    assert half.attn_dropout.hp.tolist()[:2] == [128, 0x40000000]
    assert not torch.equal(half.flat.params, plain.flat.params)
    _, again = _run({"attn_dropout": True}, 4, 3, attn_dropout=0.5)
    assert torch.equal(again.flat.params, half.flat.params) and torch.equal(again.losses(), half.losses())
    with pytest.raises(ValueError):
        half.set_hparams(attn_dropout=1.0)
    # both dropouts, each routed to its own state, keyed by the same dropout_seed
    _, both = _run({"attn_dropout": True, "dropout": True, "dropout_seed": 9}, 4, 3, attn_dropout=0.5, dropout=0.25)
    assert both.attn_dropout.host == {"attn_dropout": 0.5} and both.dropout.host == {"dropout": 0.25}
    assert both.attn_dropout.key == both.dropout.key == (9, 0)
    assert not torch.equal(both.flat.params, half.flat.params)
    _, resid = _run({"dropout": True}, 4, 3, attn_dropout=0.5, dropout=0.25)
    assert resid.attn_dropout is None


def test_program_keys_and_rejections():
    from polyaxon_amd.polyflow.executor import ResidentTrialExecutor
    from polyaxon_amd.polyflow.programs import build_program
    from polyaxon_amd.trainers import MLP

    plain = build_program("gpt2_tiny", {}, "cpu")
    prog = build_program("gpt2_tiny", {"attn_dropout": True}, "cpu")
    assert prog.hp_keys == plain.hp_keys + ("attn_dropout",) and prog.info["attn_dropout"] is True
    assert "attn_dropout" not in plain.hp_keys and "attn_dropout" not in plain.info
    assert prog.info["warm_hparams"]["attn_dropout"] == 0.1 and "attn_dropout" not in plain.info["warm_hparams"]
    assert "dropout" not in prog.hp_keys and prog.executor.dropout is None
    both = build_program("gpt2_tiny", {"attn_dropout": True, "dropout": True}, "cpu")
    assert both.hp_keys == plain.hp_keys + ("dropout", "attn_dropout")
    prog.warm(steps=1)  # warms at 0.1 and returns to 0
    assert prog.executor.attn_dropout.host == {"attn_dropout": 0.0} and prog.executor.attn_dropout.hp.tolist()[0] == 0
    assert build_program("gpt2_tiny", {"heads": 1}, "cpu").executor.model.cfg.head_dim == 64
    for name in ("resnet_tiny", "mlp"):
        with pytest.raises(ValueError, match="attn_dropout"):
            build_program(name, {"attn_dropout": True}, "cpu")
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(8, 784, generator=g), torch.randint(0, 10, (8,), generator=g))
    with pytest.raises(ValueError, match="set_attn_dropout"):
        ResidentTrialExecutor(MLP(hidden=16), batch, "cpu", channels_last=False, attn_dropout=True)


def test_example_file_searches_both_dropouts():
    import yaml

    from polyaxon_amd.polyflow.programs import build_program
    from polyaxon_amd.spec import specification_for

    path = os.path.join(ROOT, "examples", "gpt2_bo_attn_drop.yml")
    with open(path) as f:
        spec = yaml.safe_load(f)
    matrix = spec["hptuning"]["matrix"]
    assert set(matrix) == {"lr", "dropout", "attn_dropout"} and "bo" in spec["hptuning"]
    for name in ("dropout", "attn_dropout"):
        lo, hi = matrix[name]["uniform"]
        assert 0.0 <= lo < hi < 1.0
    assert set(matrix) <= set(build_program("gpt2_tiny", {"dropout": True, "attn_dropout": True}, "cpu").hp_keys)
    with open(path) as f:
        assert specification_for(f.read()).kind == "group"


def test_lm_trainer_takes_the_flag(monkeypatch):
    from polyaxon_amd import trainers
    from polyaxon_amd.ops import attn_dropout as ad

    for k in ("PLX_ZERO1", "PLX_OPT_IN_BACKWARD", "POLYAXON_DECLARATIONS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(trainers, "_tracker", lambda: None)
    built = []
    real = ad.AttnDropoutState.__init__
    monkeypatch.setattr(ad.AttnDropoutState, "__init__", lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    lm = ["--cpu", "--model", "tiny", "--steps", "2", "--log_every", "1", "--seq", "16", "--bs", "2"]
    a = trainers.train_lm(lm)
    b = trainers.train_lm(lm + ["--attn-dropout", "0"])
    assert not built                                      # at 0 no state is built
    c = trainers.train_lm(lm + ["--attn-dropout", "0.5"])
    d = trainers.train_lm(lm + ["--attn_dropout", "0.5"])
    assert a == b and c != a and c == d and len(built) == 2
