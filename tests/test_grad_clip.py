"""Global-norm gradient clipping as a device-resident hyper-parameter (ops/optim.py ``max_grad_norm``): the CPU
reference path of the fused optimizers against torch, the skip of a non-finite step, the exclusion of per-bucket
updates, and the executor / program / trainer plumbing."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn


class _Net(nn.Module):
    """One matrix (weight-decayed segment) and one bias (the tail)."""

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(24, 10)

    def forward(self, x):
        return self.fc(x)


def _data(step):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(16, 24, generator=g) * 3, torch.randint(0, 10, (16,), generator=g)


def _flat_net(seed=0):
    from polyaxon_amd.ops.flat import FlatParams

    torch.manual_seed(seed)
    net = _Net()
    ref = _Net()
    ref.load_state_dict(net.state_dict())
    return net, FlatParams(net, "cpu", channels_last=False), ref


def _first_norm():
    net, flat, _ = _flat_net()
    x, y = _data(0)
    nn.functional.cross_entropy(net(x), y).backward()
    return float(flat.grads.norm())


def _run(opt, net, steps=3):
    for s in range(steps):
        x, y = _data(s)
        nn.functional.cross_entropy(net(x), y).backward()
        opt.step_()
        opt.step += 1


def _run_torch(opt, net, c, steps=3):
    for s in range(steps):
        x, y = _data(s)
        opt.zero_grad()
        nn.functional.cross_entropy(net(x), y).backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), c)
        opt.step()


def _pair(kind, flat, ref, c):
    """The fused optimizer with max_grad_norm=c and the torch optimizer it has to follow after clip_grad_norm_."""
    from polyaxon_amd.ops.optim import FusedAdamW, FusedSGD

    if kind == "adamw":
        opt = FusedAdamW(flat, lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, max_grad_norm=c)
        topt = torch.optim.AdamW([{"params": [ref.fc.weight], "weight_decay": 0.1},
                                  {"params": [ref.fc.bias], "weight_decay": 0.0}], lr=1e-2, betas=(0.9, 0.95), eps=1e-8)
    else:
        opt = FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-2, max_grad_norm=c)
        topt = torch.optim.SGD([{"params": [ref.fc.weight], "weight_decay": 1e-2},
                                {"params": [ref.fc.bias], "weight_decay": 0.0}], lr=0.05, momentum=0.9)
    return opt, topt


@pytest.mark.parametrize("active", [True, False])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clipped_optimizers_match_torch(kind, active):
    """3 steps of clip_grad_norm_ + torch.optim on one matrix and one bias, with the threshold below the first
    step's norm (clipping active) and far above it (inactive)."""
    n0 = _first_norm()
    c = 0.3 * n0 if active else 1e3 * n0
    net, flat, ref = _flat_net()
    opt, topt = _pair(kind, flat, ref, c)
    _run(opt, net, steps=1)
    st = opt.clip_stats()
    assert st["grad_norm"] == pytest.approx(n0, rel=1e-6)
    assert (st["scale"] == pytest.approx(c / n0, rel=1e-5)) if active else (st["scale"] == 1.0)
    assert st["skipped"] == 0
    net, flat, ref = _flat_net()
    opt, topt = _pair(kind, flat, ref, c)
    _run(opt, net)
    _run_torch(topt, ref, c)
    torch.testing.assert_close(flat.master("fc.weight"), ref.fc.weight.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(flat.master("fc.bias"), ref.fc.bias.detach(), rtol=1e-5, atol=1e-6)
    assert float(flat.grads.abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clipping_is_off_by_default_and_scale_one_is_a_noop(kind):
    from polyaxon_amd.ops.optim import FusedAdamW, FusedSGD

    cls = FusedAdamW if kind == "adamw" else FusedSGD
    net, flat, _ = _flat_net()
    plain = cls(flat, lr=1e-2)
    assert "max_grad_norm" not in plain.HP and plain.HP == cls.HP
    with pytest.raises(KeyError):
        plain.set_hparams(max_grad_norm=1.0)
    with pytest.raises(RuntimeError):
        plain.grad_norm()
    _run(plain, net)
    net2, flat2, _ = _flat_net()
    clip = cls(flat2, lr=1e-2, max_grad_norm=0.0)
    assert clip.HP == cls.HP + ("max_grad_norm",) and "max_grad_norm" not in cls.HP
    assert float(clip.hp[5]) == 0.0
    clip.set_hparams(max_grad_norm=2.5)  # per trial, the usual hp copy
    assert float(clip.hp[5]) == 2.5 and float(clip.hp[0]) == pytest.approx(1e-2)
    clip.set_hparams(max_grad_norm=0.0)
    _run(clip, net2)
    assert torch.equal(flat.params, flat2.params)  # bitwise: a scale of exactly 1.0 does not perturb the gradient
    for a, b in zip(plain.state_buffers().values(), clip.state_buffers().values()):
        assert torch.equal(a, b)
    st = clip.clip_stats()
    assert st["scale"] == 1.0 and st["grad_norm"] > 0 and st["skipped"] == 0
    assert set(clip.state_buffers()) == set(plain.state_buffers())  # snapshots do not grow
    clip.reset_state()
    assert float(clip.grad_norm()) == 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_non_finite_step_is_skipped(kind, bad):
    from polyaxon_amd.ops.optim import FusedAdamW, FusedSGD

    cls = FusedAdamW if kind == "adamw" else FusedSGD
    net, flat, _ = _flat_net()
    opt = cls(flat, lr=1e-2, max_grad_norm=1.0)
    _run(opt, net, steps=1)
    p0 = flat.params.clone()
    s0 = {k: v.clone() for k, v in opt.state_buffers().items()}
    x, y = _data(1)
    nn.functional.cross_entropy(net(x), y).backward()
    flat.grads[7] = bad
    opt.step_()
    opt.step += 1
    assert torch.equal(flat.params, p0)
    for k, v in opt.state_buffers().items():
        assert torch.equal(v, s0[k]), k
    assert float(flat.grads.abs().max()) == 0.0
    st = opt.clip_stats()
    assert st["skipped"] == 1 and st["scale"] == 0.0
    _run(opt, net, steps=1)  # the next clean step updates normally
    assert not torch.equal(flat.params, p0) and bool(torch.isfinite(flat.params).all())
    st = opt.clip_stats()
    assert st["skipped"] == 1 and 0.0 < st["scale"] <= 1.0
    opt.reset_state()
    assert opt.clip_stats() == {"grad_norm": 0.0, "scale": 0.0, "skipped": 0.0}


def test_per_bucket_updates_are_excluded(capsys):
    from polyaxon_amd.ops.optim import FusedAdamW
    from polyaxon_amd.parallel.ddp import FlatDDP
    from polyaxon_amd.trainers import train_lm

    _, flat, _ = _flat_net()
    opt = FusedAdamW(flat, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatDDP(flat, optimizer=opt)
    assert opt.in_backward is False
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatDDP(flat, optimizer=opt, shard_optimizer=True)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step_range_(0, 4)
    with pytest.raises(SystemExit) as e:
        train_lm(["--cpu", "--model", "tiny", "--steps", "2", "--max_grad_norm", "1", "--zero1"])
    assert e.value.code == 2  # argparse error
    assert "max_grad_norm" in capsys.readouterr().err


@pytest.mark.parametrize("env", ["PLX_ZERO1", "PLX_OPT_IN_BACKWARD"])
def test_trainer_rejects_in_backward_env_with_clipping(env, monkeypatch):
    from polyaxon_amd.trainers import train_lm

    monkeypatch.setenv(env, "1")
    with pytest.raises(SystemExit) as e:
        train_lm(["--cpu", "--model", "tiny", "--steps", "2", "--max_grad_norm", "1"])
    assert e.value.code == 2


def test_trainer_runs_with_clipping(capsys, monkeypatch):
    import json
    import math

    from polyaxon_amd.trainers import train_lm

    for k in ("PLX_ZERO1", "PLX_OPT_IN_BACKWARD", "POLYAXON_DECLARATIONS"):
        monkeypatch.delenv(k, raising=False)
    loss = train_lm(["--cpu", "--model", "tiny", "--steps", "3", "--max_grad_norm", "0.5"])
    assert math.isfinite(loss)
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["grad_norm"] > 0 and out["skipped_steps"] == 0
    # a declared max_grad_norm (a Polyaxonfile matrix entry) reaches the same flag
    monkeypatch.setenv("POLYAXON_DECLARATIONS", json.dumps({"max_grad_norm": 0.5}))
    loss2 = train_lm(["--cpu", "--model", "tiny", "--steps", "3"])
    out2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert loss2 == loss and out2["grad_norm"] == out["grad_norm"]
    # off by default: no clip fields in the result line
    monkeypatch.delenv("POLYAXON_DECLARATIONS")
    train_lm(["--cpu", "--model", "tiny", "--steps", "3"])
    out3 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "grad_norm" not in out3 and "skipped_steps" not in out3


def test_resident_program_clips_per_trial():
    import math

    from polyaxon_amd.polyflow.programs import build_program

    plain = build_program("gpt2_tiny", {}, "cpu")
    assert plain.hp_keys == ("lr", "beta1", "beta2", "eps", "weight_decay")
    assert "max_grad_norm" not in plain.info["warm_hparams"]
    for name, keys in (("mlp", ("lr", "momentum", "weight_decay")),
                       ("resnet_tiny", ("lr", "momentum", "weight_decay", "nesterov"))):
        p = build_program(name, {"clip_grad": True}, "cpu")
        assert p.hp_keys == keys + ("max_grad_norm",) and "max_grad_norm" in p.info["warm_hparams"]
    prog = build_program("gpt2_tiny", {"clip_grad": True}, "cpu")
    assert prog.hp_keys == plain.hp_keys + ("max_grad_norm",)
    assert prog.info["warm_hparams"]["max_grad_norm"] > 0
    ex = prog.executor
    moved = {}
    for c in (1e-3, 0.0):
        ex.reset(seed=5)
        counter = getattr(ex.data, "counter", None)
        if counter is not None:
            counter.zero_()
        ex.set_hparams(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.0, max_grad_norm=c)
        p0 = ex.flat.params.clone()
        ex.run(2)
        moved[c] = float((ex.flat.params - p0).norm())
        gn = float(ex.grad_norm())
        assert math.isfinite(gn) and gn > 0
        assert (ex.clip_stats()["scale"] < 1.0) == (c > 0)
    assert 0 < moved[1e-3] < moved[0.0]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from polyaxon_amd.models.transformer import Transformer, lm_loss, tiny_llama
    from polyaxon_amd.ops.flat import FlatParams
    from polyaxon_amd.ops.optim import FusedAdamW
    from polyaxon_amd.parallel.ddp import FlatDDP, init_from_env

    init_from_env("gloo")
    torch.manual_seed(0)
    model = Transformer(tiny_llama())
    flat = FlatParams(model, "cpu", channels_last=False)
    opt = FusedAdamW(flat, lr=1e-2, weight_decay=0.1, max_grad_norm=0.5)
    ddp = FlatDDP(flat, bucket_mb=0.01)  # plain: all-reduce, then step_()
    ddp.broadcast_params()
    gen = torch.Generator().manual_seed(100 + rank)  # different data per rank
    norms, scales = [], []
    for _ in range(3):
        tokens = torch.randint(0, 256, (4, 16), generator=gen)
        lm_loss(model(tokens), tokens).backward()
        ddp.finish()
        opt.step_()
        opt.step += 1
        st = opt.clip_stats()
        norms.append(st["grad_norm"])
        scales.append(st["scale"])
    q.put((rank, norms, scales, flat.params.numpy().copy()))
    dist.destroy_process_group()


def test_plain_flat_ddp_with_clipping_gloo_world2():
    """Every rank norms the same averaged gradients: the same grad_norm every step, bitwise-equal parameters."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    assert res[0][1] == res[1][1] and all(n > 0 for n in res[0][1])
    assert res[0][2] == res[1][2] and min(res[0][2]) < 1.0  # clipping was active
    assert (res[0][3] == res[1][3]).all()
