"""Label smoothing and z-loss as device-resident loss hyper-parameters (ops/loss_hp.py, ops/lm.py ``loss_hp=``) on the
CPU path: validation, the torch fallback of both cross entropies against the formulas in float64, the executor /
program plumbing, the example file, and the torch-free import."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPS = [(0.0, 0.0), (0.1, 0.0), (0.0, 1e-3), (0.2, 1e-4)]


def test_validate():
    from polyaxon_amd.ops import loss_hp

    assert loss_hp.KEYS == ("label_smoothing", "z_loss")
    assert loss_hp.DEFAULTS == {"label_smoothing": 0.0, "z_loss": 0.0}
    for v in (0, 0.1, 0.999):
        assert loss_hp.validate("label_smoothing", v) == float(v)
    assert loss_hp.validate("z_loss", 0) == 0.0 and loss_hp.validate("z_loss", 1e-4) == 1e-4
    for key, v in (("label_smoothing", 1.0), ("label_smoothing", -0.1), ("label_smoothing", float("nan")),
                   ("label_smoothing", float("inf")), ("z_loss", -1e-4), ("z_loss", float("nan")),
                   ("z_loss", float("inf"))):
        with pytest.raises(ValueError, match=key):
            loss_hp.validate(key, v)


def test_set_merges_and_rejects_whole_calls():
    from polyaxon_amd.ops.loss_hp import LossHParams

    h = LossHParams("cpu")
    assert h.hp.tolist() == [0.0, 0.0, 0.0, 0.0] and h.nll.dim() == 0 and h.nll.dtype == torch.float32
    h.set(label_smoothing=0.25)
    h.set(z_loss=0.5)
    assert h.hp.tolist() == [0.25, 0.5, 0.0, 0.0] and h.host == {"label_smoothing": 0.25, "z_loss": 0.5}
    with pytest.raises(ValueError):
        h.set(z_loss=0.125, label_smoothing=1.0)  # its valid key is not applied either
    assert h.hp.tolist() == [0.25, 0.5, 0.0, 0.0]
    with pytest.raises(KeyError):
        h.set(lr=0.1)


def _ref64(x, y, C, eps, zeta, rows_mean):
    """The formulas in float64 with autograd: per valid row (target in [0, C)) nll = l - x_t and
    loss = l - (1 - eps) x_t - eps mean_{j<C} x_j + zeta l^2, l over all V columns; divided by every row
    (``rows_mean``) or by the valid ones.  Returns (loss, nll, dloss/dx)."""
    x = x.double().requires_grad_()
    valid = (y >= 0) & (y < C)
    l = torch.logsumexp(x, dim=-1)
    xt = x.gather(1, torch.where(valid, y, torch.zeros_like(y))[:, None])[:, 0]
    nll = torch.where(valid, l - xt, torch.zeros_like(l))
    loss = torch.where(valid, l - (1 - eps) * xt - eps * x[:, :C].mean(-1) + zeta * l * l, torch.zeros_like(l))
    rows = y.numel() if rows_mean else max(1, int(valid.sum()))
    loss, nll = loss.sum() / rows, nll.sum() / rows
    (g,) = torch.autograd.grad(loss * 1.7, x)
    return float(loss.detach()), float(nll.detach()), g


def _inputs(N, V, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, V, generator=g) * 3
    x[:, C:] = float("-inf")
    return x, torch.randint(0, C, (N,), generator=g)


def _check(got_loss, got_nll, got_grad, ref):
    # fp32 against fp64 on a few hundred terms of magnitude <= 20: far below 1e-5 relative
    assert float(got_loss.detach()) == pytest.approx(ref[0], rel=1e-5, abs=1e-6)
    assert float(got_nll) == pytest.approx(ref[1], rel=1e-5, abs=1e-6)
    torch.testing.assert_close(got_grad.double(), ref[2], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("eps,zeta", HPS)
@pytest.mark.parametrize("V,C", [(11, 11), (24, 17)])
@pytest.mark.parametrize("in_range", [False, True])
def test_class_xent_fallback_matches_float64(in_range, V, C, eps, zeta):
    from polyaxon_amd.ops.lm import class_xent
    from polyaxon_amd.ops.loss_hp import LossHParams

    x, y = _inputs(9, V, C, seed=V)
    if not in_range:  # ignored: -100 and, with padding, a label in [C, V)
        y[2] = -100
        y[5] = C if C < V else -100
    h = LossHParams("cpu")
    h.set(label_smoothing=eps, z_loss=zeta)
    h.nll.fill_(-1.0)
    xin = x.clone().requires_grad_()
    loss = class_xent(xin, y, in_range=in_range, loss_hp=h, n_classes=C)
    (loss * 1.7).backward()
    _check(loss, h.nll, xin.grad, _ref64(x, y, C, eps, zeta, rows_mean=in_range))
    if not in_range:
        assert float(xin.grad[2].abs().max()) == 0.0 and float(xin.grad[5].abs().max()) == 0.0
    assert float(xin.grad[:, C:].abs().sum()) == 0.0
    if eps == 0.0 and zeta == 0.0:
        assert float(h.nll) == float(loss.detach())


@pytest.mark.parametrize("eps,zeta", HPS)
@pytest.mark.parametrize("V,C", [(11, 11), (24, 17)])
def test_next_token_xent_fallback_matches_float64(V, C, eps, zeta):
    from polyaxon_amd.ops.lm import next_token_xent
    from polyaxon_amd.ops.loss_hp import LossHParams

    B, S = 2, 5
    x, _ = _inputs(B * S, V, C, seed=100 + V)
    g = torch.Generator().manual_seed(7)
    tokens = torch.randint(0, C, (B, S), generator=g)
    tokens[0, 2] = -100
    tokens[1, 3] = C if C < V else -100
    h = LossHParams("cpu")
    h.set(label_smoothing=eps, z_loss=zeta)
    xin = x.view(B, S, V).clone().requires_grad_()
    loss = next_token_xent(xin, tokens, loss_hp=h, n_classes=C)
    (loss * 1.7).backward()
    rows = x.view(B, S, V)[:, :-1].reshape(-1, V)
    ref = _ref64(rows, tokens[:, 1:].reshape(-1), C, eps, zeta, rows_mean=True)  # the mean is over all B (S - 1) rows
    got = xin.grad[:, :-1].reshape(-1, V)
    _check(loss, h.nll, got, ref)
    assert float(xin.grad[:, -1].abs().max()) == 0.0  # the last position predicts nothing
    assert float(xin.grad[0, 1].abs().max()) == 0.0 and float(xin.grad[1, 2].abs().max()) == 0.0


def test_n_classes_is_checked():
    from polyaxon_amd.ops.lm import class_xent
    from polyaxon_amd.ops.loss_hp import LossHParams

    x, y = _inputs(3, 8, 8, seed=0)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            class_xent(x, y, loss_hp=LossHParams("cpu"), n_classes=bad)


def test_without_loss_hp_nothing_changes():
    """The guard: ``loss_hp=None`` is the call it was (this one also passes without the feature)."""
    from polyaxon_amd.models.transformer import lm_loss
    from polyaxon_amd.ops.lm import class_xent, next_token_xent

    x, y = _inputs(6, 13, 13, seed=3)
    assert torch.equal(class_xent(x, y), F.cross_entropy(x, y))
    assert torch.equal(class_xent(x, y, in_range=True), F.cross_entropy(x, y))
    x3 = x.view(2, 3, 13)
    tokens = y.view(2, 3)
    want = F.cross_entropy(x3[:, :-1].reshape(-1, 13), tokens[:, 1:].reshape(-1))
    assert torch.equal(next_token_xent(x3, tokens), want) and torch.equal(lm_loss(x3, tokens), want)


# ------------------------------------------------------------------ executor, programs
def _run(name, params, seed, steps, **hp):
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program(name, params, "cpu")
    ex = prog.executor
    ex.reset(seed=seed)
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k not in ("label_smoothing", "z_loss")}
    ex.set_hparams(**base, **hp)
    ex.run(steps)
    return prog, ex


@pytest.mark.parametrize("name", ["resnet_tiny", "gpt2_tiny"])
def test_programs_search_the_loss_per_trial(name):
    from polyaxon_amd.ops import loss_hp

    plain, ex0 = _run(name, {}, 4, 3, label_smoothing=0.2, z_loss=0.1)  # without the flag the keys are ignored
    assert not any(k in plain.hp_keys for k in loss_hp.KEYS) and "loss_hparams" not in plain.info
    assert ex0.loss_hp is None and "label_smoothing" not in plain.info["warm_hparams"]
    with pytest.raises(RuntimeError):
        ex0.train_loss()
    prog, ex1 = _run(name, {"loss_hparams": True}, 4, 3, label_smoothing=0.0, z_loss=0.0)
    assert prog.hp_keys == plain.hp_keys + loss_hp.KEYS and prog.info["loss_hparams"] is True
    assert prog.info["warm_hparams"]["label_smoothing"] == 0.1 and prog.info["warm_hparams"]["z_loss"] == 1e-4
    # at 0 / 0 the step is the plain step: the same parameters bit for bit, the same recorded losses
    assert torch.equal(ex1.flat.params, ex0.flat.params)
    assert torch.equal(ex1.losses(), ex0.losses())
    assert float(ex1.train_loss()) == float(ex1.losses()[-1])
    # a smoothed trial trains on another loss, and the ring still holds the plain NLL
    _, ex2 = _run(name, {"loss_hparams": True}, 4, 1, label_smoothing=0.2)
    assert ex2.loss_hp.hp.tolist() == pytest.approx([0.2, 0.0, 0.0, 0.0])
    assert float(ex2.losses()[0]) == float(ex1.losses()[0])  # same weights, same batch: the same NLL
    # (the smoothed loss exceeds the NLL by eps x (x_t - mean_j x_j) averaged over the rows: 1e-2 .. 4e-2 here)
    assert float(ex2.train_loss()) > float(ex2.losses()[0])
    ex2.run(2)
    assert not torch.equal(ex2.flat.params, ex1.flat.params)
    with pytest.raises(ValueError):
        ex2.set_hparams(label_smoothing=1.0)


def test_warm_returns_the_loss_to_plain():
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("resnet_tiny", {"loss_hparams": True}, "cpu")
    prog.warm(steps=1)
    assert prog.executor.loss_hp.hp.tolist() == [0.0, 0.0, 0.0, 0.0]
    assert prog.executor.loss_hp.host == {"label_smoothing": 0.0, "z_loss": 0.0}


def test_custom_loss_fn_receives_loss_hp():
    from polyaxon_amd.polyflow.executor import ResidentTrialExecutor
    from polyaxon_amd.trainers import MLP

    seen = []

    def loss_fn(out, y, loss_hp=None):
        seen.append(loss_hp)
        return F.cross_entropy(out, y)

    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(8, 784, generator=g), torch.randint(0, 10, (8,), generator=g))
    ex = ResidentTrialExecutor(MLP(hidden=16), batch, "cpu", loss_fn=loss_fn, channels_last=False, loss_hparams=True)
    ex.reset(seed=0)
    ex.run(1)
    assert seen == [ex.loss_hp]


def test_trainers_take_the_flags(capsys, monkeypatch):
    import json

    from polyaxon_amd import trainers

    for k in ("PLX_ZERO1", "PLX_OPT_IN_BACKWARD", "POLYAXON_DECLARATIONS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(trainers, "_tracker", lambda: None)
    args = ["--cpu", "--bs", "2", "--image", "32", "--units", "1", "--unit_steps", "1", "--lr", "0.05"]
    trainers.train_resnet(args)
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "train_loss" not in plain
    monkeypatch.setenv("POLYAXON_DECLARATIONS", json.dumps({"label_smoothing": 0.2}))
    trainers.train_resnet(args)
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["train_loss"] > out["loss"] == plain["loss"]  # one step: the same weights, the same plain NLL
    monkeypatch.delenv("POLYAXON_DECLARATIONS")
    lm = ["--cpu", "--model", "tiny", "--steps", "2", "--log_every", "1", "--seq", "16", "--bs", "2"]
    a = trainers.train_lm(lm)
    b = trainers.train_lm(lm + ["--label_smoothing", "0", "--z_loss", "0"])
    c = trainers.train_lm(lm + ["--label_smoothing", "0.1", "--z_loss", "1e-4"])
    assert a == b and c != a and abs(c - a) < 0.5  # the reported loss is the plain NLL of a differently trained model


def test_example_file_searches_label_smoothing():
    import yaml

    from polyaxon_amd.ops import loss_hp
    from polyaxon_amd.polyflow.programs import PROGRAMS, build_program
    from polyaxon_amd.spec import specification_for

    path = os.path.join(ROOT, "examples", "resnet50_hyperband_smooth.yml")
    with open(path) as f:
        spec = yaml.safe_load(f)
    ex = spec["environment"]["executor"]
    assert ex["kind"] == "resident" and ex["program"] == "resnet50" and ex["program"] in PROGRAMS
    assert ex["params"]["loss_hparams"] is True
    matrix = spec["hptuning"]["matrix"]
    assert matrix["label_smoothing"] == {"uniform": [0.0, 0.2]} and "hyperband" in spec["hptuning"]
    # the same builder at CPU-test size understands every searched key
    prog = build_program("resnet_tiny", {"loss_hparams": True}, "cpu")
    assert set(matrix) <= set(prog.hp_keys) and set(loss_hp.KEYS) <= set(prog.hp_keys)
    with open(path) as f:
        assert specification_for(f.read()).kind == "group"


def test_loss_hp_module_is_torch_free():
    code = ("import sys; import polyaxon_amd.ops.loss_hp as m; import polyaxon_amd.polyflow.programs; "
            "assert m.validate('z_loss', 1) == 1.0; assert 'torch' not in sys.modules, 'torch was imported'")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
