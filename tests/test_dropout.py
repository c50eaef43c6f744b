"""Residual dropout as a device-resident hyper-parameter (ops/dropout.py) on the CPU path: threshold / scale /
validation, the torch-free import, the statistics of the mask's numpy twin, the gpt2_tiny program through
``build_program`` (bitwise the plain step at rate 0, reproducible, resumable from a snapshot, the same masks for every
trial), the program keys and the example file."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. threshold, scale, validation
def test_threshold_scale_validate():
    from polyaxon_amd.ops import dropout

    assert dropout.KEYS == ("dropout",) and dropout.DEFAULTS == {"dropout": 0.0}
    assert dropout.threshold(0) == 0 and dropout.scale(0) == 1.0
    assert dropout.threshold(0.1) == 6554
    assert dropout.threshold(0.5) == 32768 and dropout.scale(32768) == 2.0
    assert dropout.threshold(0.9999999) == 65535 and dropout.scale(65535) == 65536.0
    # fp64 quotient rounded once to fp32
    assert dropout.scale(6554) == float(np.float32(65536.0 / (65536 - 6554)))
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="dropout"):
            dropout.validate("dropout", bad)
    with pytest.raises(KeyError):
        dropout.validate("lr", 0.1)


def test_set_uploads_the_four_words_and_rejects_whole_calls():
    from polyaxon_amd.ops.dropout import DropoutState

    step = torch.zeros(1, dtype=torch.int32)
    st = DropoutState("cpu", step, seed=(7 << 32) | 0x80000001, rank=3)
    assert st.hp.dtype == torch.int32 and st.hp.shape == (4,)
    words = [w & 0xFFFFFFFF for w in st.hp.tolist()]
    assert words == [0, 0x3F800000, 0x80000001, 7 ^ 3]  # T = 0, c = 1.0f, the key with the rank in its second word
    st.set(dropout=0.1)
    want = [6554, int(np.float32(65536.0 / (65536 - 6554)).view(np.uint32)), 0x80000001, 4]
    assert [w & 0xFFFFFFFF for w in st.hp.tolist()] == want and st.host == {"dropout": 0.1}
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            st.set(dropout=bad)
        assert [w & 0xFFFFFFFF for w in st.hp.tolist()] == want and st.host == {"dropout": 0.1}
    step += 5
    assert st.step() == 5


# ------------------------------------------------------------------ 2. torch-free import
def test_dropout_module_is_torch_free():
    code = ("import sys; import polyaxon_amd.ops.dropout as m; import polyaxon_amd.polyflow.programs; "
            "assert m.threshold(0.1) == 6554; assert 'torch' not in sys.modules, 'torch was imported'")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ------------------------------------------------------------------ 3. mask statistics
N_VEC = 1 << 17


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_mask_statistics(p):
    """Dropped counts (all 2^20 elements and each of the 8 lanes) within 5 binomial sigma of N T / 65536; agreement
    with the mask of the next step, the next site and the next key within 5 sigma of q^2 + (1 - q)^2, what two
    independent masks of rate q agree on."""
    from polyaxon_amd.ops import dropout

    T = dropout.threshold(p)
    q = T / 65536.0
    base = dropout.mask_reference((0, 0), 3, 2, N_VEC, T)
    assert base.shape == (N_VEC, 8) and base.dtype == np.bool_
    n = base.size
    z = abs(int((~base).sum()) - n * q) / math.sqrt(n * q * (1 - q))
    print(f"p={p} dropped z={z:.2f}")
    assert z <= 5.0
    for lane in range(8):
        z = abs(int((~base[:, lane]).sum()) - N_VEC * q) / math.sqrt(N_VEC * q * (1 - q))
        print(f"p={p} lane {lane} z={z:.2f}")
        assert z <= 5.0
    a = q * q + (1 - q) * (1 - q)
    others = {"step": dropout.mask_reference((0, 0), 4, 2, N_VEC, T),
              "site": dropout.mask_reference((0, 0), 3, 3, N_VEC, T),
              "key": dropout.mask_reference((1, 0), 3, 2, N_VEC, T)}
    for name, other in others.items():
        z = abs(int((other == base).sum()) - n * a) / math.sqrt(n * a * (1 - a))
        print(f"p={p} agreement with next {name} z={z:.2f}")
        assert z <= 5.0


def test_mask_edges():
    from polyaxon_amd.ops import dropout

    assert dropout.mask_reference((0, 0), 0, 0, 64, 0).all()  # T = 0 keeps everything
    m = dropout.mask_reference((5, 6), 9, 1, 4096, 65535)      # T = 65535 keeps only the half 0xffff
    assert 0 <= int(m.sum()) < 8
    # a prefix of a longer mask: the draw of a vector depends on its index alone
    assert np.array_equal(dropout.mask_reference((5, 6), 9, 1, 100, 6554),
                          dropout.mask_reference((5, 6), 9, 1, 4096, 6554)[:100])


# ------------------------------------------------------------------ 4. gpt2_tiny through build_program
def _run(params, seed, steps, **hp):
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("gpt2_tiny", params, "cpu")
    ex = prog.executor
    ex.reset(seed=seed)
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k != "dropout"}
    ex.set_hparams(**base, **hp)
    ex.run(steps)
    return prog, ex


def test_gpt2_tiny_rate_zero_is_the_plain_step_and_trials_reproduce():
    _, plain = _run({}, 4, 3, dropout=0.5)  # without the param the key is dropped
    assert plain.dropout is None
    _, zero = _run({"dropout": True}, 4, 3, dropout=0.0)
    assert torch.equal(zero.flat.params, plain.flat.params) and torch.equal(zero.losses(), plain.losses())
    _, half = _run({"dropout": True}, 4, 3, dropout=0.5)
    assert not torch.equal(half.flat.params, plain.flat.params)
    _, again = _run({"dropout": True}, 4, 3, dropout=0.5)
    assert torch.equal(again.flat.params, half.flat.params) and torch.equal(again.losses(), half.losses())
    with pytest.raises(ValueError):
        half.set_hparams(dropout=1.0)


def test_gpt2_tiny_continues_its_masks_from_a_snapshot():
    """The snapshot holds the step counter and no dropout memory: the restored trial redraws the masks of steps 2
    and 3.  The token stream has a counter of its own that snapshots do not cover; it is rewound by hand so both
    runs read the same batches."""
    _, ex = _run({"dropout": True, "dropout_seed": 11}, 4, 2, dropout=0.5)
    ex.snapshot("rung")
    c0 = ex.data.counter.clone()
    ex.run(2)
    first = ex.flat.params.clone()
    ex.restore("rung")
    ex.data.counter.copy_(c0)
    ex.run(2)
    assert int(ex.step.item()) == 4 and torch.equal(ex.flat.params, first)


def test_every_trial_sees_the_same_masks(monkeypatch):
    from polyaxon_amd.ops import dropout
    from polyaxon_amd.polyflow.programs import build_program

    log = []
    real = dropout.mask_reference

    def logged(key, step, site, n_vec, T):
        m = real(key, step, site, n_vec, T)
        log.append((tuple(key), int(step), int(site), int(n_vec), int(T), m.tobytes()))
        return m

    monkeypatch.setattr(dropout, "mask_reference", logged)
    prog = build_program("gpt2_tiny", {"dropout": True, "dropout_seed": 5}, "cpu")
    ex = prog.executor
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k != "dropout"}
    runs = []
    for seed in (1, 2):
        ex.reset(seed=seed)
        ex.set_hparams(**base, dropout=0.3)
        del log[:]
        ex.run(2)
        runs.append((list(log), ex.flat.params.clone()))
    (log1, p1), (log2, p2) = runs
    assert not torch.equal(p1, p2)  # other weights ...
    assert log1 == log2             # ... the same masks at the same steps
    n_layers = ex.model.cfg.n_layers
    assert {e[0] for e in log1} == {(5, 0)} and {e[4] for e in log1} == {dropout.threshold(0.3)}
    assert {e[1] for e in log1} == {0, 1}
    assert {e[2] for e in log1} == set(range(2 * n_layers + 1))  # every residual site and the embedding sum
    assert len({e[5] for e in log1}) == len(log1)  # no two (step, site) draws coincide


def test_eval_and_no_state_are_the_plain_path(monkeypatch):
    from polyaxon_amd.models.transformer import Transformer, gpt2_125m
    from polyaxon_amd.ops import dropout

    torch.manual_seed(0)
    model = Transformer(gpt2_125m(vocab_size=64, n_layers=2, d_model=32, n_heads=2, d_ff=64, max_seq_len=16))
    tokens = torch.randint(0, 64, (2, 16))
    model.train()
    plain = model(tokens)
    st = dropout.DropoutState("cpu", torch.zeros(1, dtype=torch.int32), seed=1)
    st.set(dropout=0.5)
    model.set_dropout(st)
    assert not torch.equal(model(tokens), plain)
    model.eval()
    monkeypatch.setattr(dropout, "mask_reference", lambda *a: pytest.fail("a mask was drawn in eval()"))
    assert torch.equal(model(tokens), plain)
    model.train()
    model.set_dropout(None)
    assert torch.equal(model(tokens), plain)


def test_checkpointed_blocks_draw_the_masks_of_the_fused_loop():
    """Block.forward (the activation-checkpoint path) and the fused add + norm loop drop the same elements: the same
    loss and the same gradients up to fp32 summation order."""
    from polyaxon_amd.models.transformer import Transformer, gpt2_125m, lm_loss
    from polyaxon_amd.ops import dropout

    kw = dict(vocab_size=64, n_layers=2, d_model=32, n_heads=2, d_ff=64, max_seq_len=16)
    torch.manual_seed(0)
    a = Transformer(gpt2_125m(**kw))
    b = Transformer(gpt2_125m(checkpoint=True, **kw))
    b.load_state_dict(a.state_dict())
    tokens = torch.randint(0, 64, (2, 16))
    st = dropout.DropoutState("cpu", torch.zeros(1, dtype=torch.int32), seed=2)
    st.set(dropout=0.4)
    grads = []
    for m in (a, b):
        m.train()
        m.set_dropout(st)
        loss = lm_loss(m(tokens), tokens)
        loss.backward()
        grads.append((loss.detach(), m.blocks[0].attn.qkv.weight.grad.clone()))
    torch.testing.assert_close(grads[0][0], grads[1][0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(grads[0][1], grads[1][1], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------ 5. program keys, the example
def test_program_keys_and_rejections():
    from polyaxon_amd.polyflow.executor import ResidentTrialExecutor
    from polyaxon_amd.polyflow.programs import build_program
    from polyaxon_amd.trainers import MLP

    plain = build_program("gpt2_tiny", {}, "cpu")
    prog = build_program("gpt2_tiny", {"dropout": True}, "cpu")
    assert prog.hp_keys == plain.hp_keys + ("dropout",) and prog.info["dropout"] is True
    assert "dropout" not in plain.hp_keys and "dropout" not in plain.info
    assert prog.info["warm_hparams"]["dropout"] == 0.1 and "dropout" not in plain.info["warm_hparams"]
    prog.warm(steps=1)  # warms at 0.1 and returns to 0
    assert prog.executor.dropout.host == {"dropout": 0.0} and prog.executor.dropout.hp.tolist()[0] == 0
    for name in ("resnet_tiny", "mlp"):
        with pytest.raises(ValueError, match="dropout"):
            build_program(name, {"dropout": True}, "cpu")
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(8, 784, generator=g), torch.randint(0, 10, (8,), generator=g))
    with pytest.raises(ValueError, match="set_dropout"):
        ResidentTrialExecutor(MLP(hidden=16), batch, "cpu", channels_last=False, dropout=True)


def test_example_file_searches_dropout():
    import yaml

    from polyaxon_amd.polyflow.programs import build_program
    from polyaxon_amd.spec import specification_for

    path = os.path.join(ROOT, "examples", "gpt2_bo_drop.yml")
    with open(path) as f:
        spec = yaml.safe_load(f)
    matrix = spec["hptuning"]["matrix"]
    assert set(matrix) == {"lr", "dropout"} and "bo" in spec["hptuning"]
    lo, hi = matrix["dropout"]["uniform"]
    assert 0.0 <= lo < hi < 1.0
    assert set(matrix) <= set(build_program("gpt2_tiny", {"dropout": True}, "cpu").hp_keys)
    with open(path) as f:
        assert specification_for(f.read()).kind == "group"


def test_lm_trainer_takes_the_flag(monkeypatch):
    from polyaxon_amd import trainers

    for k in ("PLX_ZERO1", "PLX_OPT_IN_BACKWARD", "POLYAXON_DECLARATIONS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(trainers, "_tracker", lambda: None)
    lm = ["--cpu", "--model", "tiny", "--steps", "2", "--log_every", "1", "--seq", "16", "--bs", "2"]
    a = trainers.train_lm(lm)
    b = trainers.train_lm(lm + ["--dropout", "0"])
    c = trainers.train_lm(lm + ["--dropout", "0.5"])
    d = trainers.train_lm(lm + ["--dropout", "0.5"])
    assert a == b and c != a and c == d
