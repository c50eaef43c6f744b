"""Device-resident learning-rate schedules (ops/optim.py ``lr_schedule``) on the CPU path: the float32 twin of the
``plx_lr_schedule`` kernel against a float64 reference, the fused optimizers' scheduled trajectory against a
host-set LR, validation, composition with clipping and per-bucket updates, resume, and the executor / program /
sweep / trainer / example plumbing."""
import json
import math

import pytest
import torch
import torch.nn as nn

KINDS = ("constant", "linear", "cosine", "step", "inv_sqrt")
PAIRS = [(0, 1), (0, 2), (1, 2), (3, 10), (5, 5), (7, 4), (100, 100000)]  # (W, T)
FLOORS = (0.0, 0.1, 1.0)
GAMMA = 0.5


def decay_every(T):
    """E of the ``step`` kind per (W, T) pair: gamma^k stays a normal fp32 number (k <= 99) over 0..T+5."""
    return 1 if T < 100 else 1000


def steps_of(W, T, full):
    """s over 0..T+5; the CPU twin is one Python call per step, so the long pair keeps every step within 5 of 0, W
    and T (the edges W-1, W, T-1, T and the clamp past T) and every 997th step between."""
    if full or T + 5 < 1000:
        return list(range(T + 6))
    near = set(range(0, 6)) | set(range(W - 5, W + 6)) | set(range(T - 5, T + 6)) | set(range(0, T + 6, 997))
    return sorted(s for s in near if 0 <= s <= T + 5)


def ref_factor(kind, s, W, T, m, gamma, E):
    """The issue's formula in Python float64."""
    if s < W:
        return (s + 1) / W
    if kind == "constant":
        return 1.0
    if kind in ("linear", "cosine"):
        if T <= W:
            return 1.0
        p = min(1.0, max(0.0, (s - W) / max(1, T - W)))
        return 1.0 - (1.0 - m) * p if kind == "linear" else m + (1.0 - m) * 0.5 * (1.0 + math.cos(math.pi * p))
    if kind == "step":
        return max(m, gamma ** ((s - W) // max(1, E)))
    return max(m, math.sqrt(max(W, 1) / (s + 1)))


def exactly_one(kind, s, W, T, m, gamma, E):
    """The branches on which the factor is 1 by definition, not by arithmetic."""
    if s < W:
        return s + 1 == W
    if kind == "constant":
        return True
    if kind in ("linear", "cosine"):
        return T <= W or s == W or m == 1.0
    if kind == "step":
        return (s - W) // max(1, E) == 0 or m == 1.0 or gamma == 1.0
    return m == 1.0 or s + 1 == max(W, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_lr_factor_matches_float64(kind):
    """fp32 against fp64: at most 8 roundings on magnitudes <= pi plus cos's, far below 2e-6 of the base LR; the
    ``step`` kind is gamma^k alone: relative 2e-6."""
    from polyaxon_amd.ops.optim import lr_factor

    worst = 0.0
    for W, T in PAIRS:
        E = decay_every(T)
        for m in FLOORS:
            for s in steps_of(W, T, full=False):
                f = lr_factor(kind, s, W, T, m, GAMMA, E)
                assert f.dtype == torch.float32 and f.dim() == 0
                want = ref_factor(kind, s, W, T, m, GAMMA, E)
                err = abs(float(f) - want) / (want if kind == "step" else 1.0)
                worst = max(worst, err)
                assert err <= 2e-6, (kind, W, T, m, s, float(f), want)
                if exactly_one(kind, s, W, T, m, GAMMA, E):
                    assert float(f) == 1.0, (kind, W, T, m, s)
                if kind in ("linear", "cosine") and T > W and s >= T:
                    assert float(f) == float(torch.tensor(m, dtype=torch.float32)), (kind, W, T, m, s)
    print(f"lr_factor {kind}: worst error {worst:.3g}")
    assert float(lr_factor(KINDS.index(kind), 4, 3, 10, 0.1, GAMMA, 1)) == float(lr_factor(kind, 4, 3, 10, 0.1, GAMMA, 1))


# ------------------------------------------------------------------ the fused optimizers
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


def _make(kind, flat, **kw):
    from polyaxon_amd.ops.optim import FusedAdamW, FusedSGD

    if kind == "adamw":
        return FusedAdamW(flat, lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, **kw)
    return FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-2, **kw)


def _base(kind):
    return 1e-2 if kind == "adamw" else 0.05


def _twin_lr(base, sched, s):
    """The float32 LR the schedule gives at ``s`` completed steps: fp32(base) x twin factor, one fp32 product."""
    from polyaxon_amd.ops.optim import lr_factor

    f = lr_factor(sched["lr_schedule"], s, sched["warmup_steps"], sched["lr_total_steps"], sched["min_lr_ratio"],
                  sched.get("lr_decay_gamma", 0.1), sched.get("lr_decay_every", 1))
    return float(torch.tensor(base, dtype=torch.float32) * f)


def _step(opt, net, s):
    x, y = _data(s)
    nn.functional.cross_entropy(net(x), y).backward()
    opt.step_()
    opt.step += 1


SCHEDULES = [
    {"lr_schedule": "cosine", "warmup_steps": 3, "lr_total_steps": 10, "min_lr_ratio": 0.1},
    {"lr_schedule": "linear", "warmup_steps": 2, "lr_total_steps": 12, "min_lr_ratio": 0.0},
    {"lr_schedule": "step", "warmup_steps": 1, "lr_total_steps": 0, "min_lr_ratio": 0.05, "lr_decay_gamma": 0.5,
     "lr_decay_every": 3},
    {"lr_schedule": "inv_sqrt", "warmup_steps": 4, "lr_total_steps": 0, "min_lr_ratio": 0.2},
    {"lr_schedule": "constant", "warmup_steps": 5, "lr_total_steps": 0, "min_lr_ratio": 0.0},
]


@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda s: s["lr_schedule"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_scheduled_optimizer_equals_host_set_lr_bitwise(kind, sched):
    net, flat, _ = _flat_net()
    opt = _make(kind, flat, lr_schedule="constant")
    opt.set_hparams(**sched)
    net2, flat2, _ = _flat_net()
    plain = _make(kind, flat2)
    lrs = []
    for s in range(12):
        _step(opt, net, s)
        lrs.append(float(opt.current_lr()))
        plain.set_hparams(lr=_twin_lr(_base(kind), sched, s))
        _step(plain, net2, s)
        assert lrs[-1] == float(plain.hp[0]), (s, lrs[-1], float(plain.hp[0]))
    assert torch.equal(flat.params, flat2.params)
    for a, b in zip(opt.state_buffers().values(), plain.state_buffers().values()):
        assert torch.equal(a, b)
    assert len(set(lrs)) > 2  # the LR did move


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_off_by_default_and_constant_is_a_noop(kind):
    from polyaxon_amd.ops import lr_schedule as lrs
    from polyaxon_amd.ops.optim import FusedAdamW, FusedSGD

    cls = FusedAdamW if kind == "adamw" else FusedSGD
    net, flat, _ = _flat_net()
    plain = _make(kind, flat, lr_schedule=None)
    assert plain.HP == cls.HP and plain._sched is None and not plain.scheduled
    assert not any(k in cls.HP for k in lrs.KEYS)
    with pytest.raises(KeyError):
        plain.set_hparams(warmup_steps=3)
    net1, flat1, _ = _flat_net()
    default = _make(kind, flat1)
    net2, flat2, _ = _flat_net()
    const = _make(kind, flat2, lr_schedule="constant")
    assert const.HP == cls.HP + lrs.KEYS and const.scheduled
    assert const.hp.numel() == 8 and const._sched.sched.numel() == 8
    assert float(const.hp[5]) == 0.0  # the schedule's keys live in `sched`: hp's slots stay what they were
    assert const._sched.sched.tolist()[1:4] == [0.0, 0.0, 0.0]
    for s in range(4):
        _step(plain, net, s)
        _step(default, net1, s)
        _step(const, net2, s)
        assert float(const.current_lr()) == float(plain.hp[0]) == float(plain.current_lr())
    assert torch.equal(flat.params, flat1.params) and torch.equal(flat.params, flat2.params)
    for a, b in zip(plain.state_buffers().values(), const.state_buffers().values()):
        assert torch.equal(a, b)
    assert set(const.state_buffers()) == set(plain.state_buffers())  # snapshots do not grow


def test_set_hparams_routes_and_validates():
    from polyaxon_amd.ops.optim import FusedAdamW

    _, flat, _ = _flat_net()
    opt = FusedAdamW(flat, lr=1e-3, lr_schedule="linear")
    assert opt._sched.sched.tolist()[1] == 1.0
    opt.set_hparams(lr=2e-3, lr_schedule="cosine", warmup_steps=7, lr_total_steps=50, min_lr_ratio=0.25,
                    lr_decay_gamma=0.5, lr_decay_every=4)
    got = opt._sched.sched.tolist()
    assert got == pytest.approx([2e-3, 2.0, 7.0, 50.0, 0.25, 0.5, 4.0, 0.0])
    opt.set_hparams(lr_schedule=4)  # a kind as its code
    assert opt._sched.sched.tolist()[1] == 4.0
    opt.set_hparams(weight_decay=0.3)  # an ordinary key leaves the schedule alone
    assert opt._sched.sched.tolist()[1:3] == [4.0, 7.0] and float(opt.hp[4]) == pytest.approx(0.3)
    before = opt._sched.sched.clone()
    bad = [{"lr_schedule": "exponential"}, {"lr_schedule": 5}, {"lr_schedule": -1}, {"lr_schedule": 1.5},
           {"warmup_steps": -1}, {"lr_total_steps": -3}, {"lr_decay_every": -1},
           {"warmup_steps": 2 ** 24}, {"lr_total_steps": 2 ** 24}, {"lr_decay_every": 2 ** 24},
           {"min_lr_ratio": -0.01}, {"min_lr_ratio": 1.01},
           {"lr_decay_gamma": 0.0}, {"lr_decay_gamma": -0.5}, {"lr_decay_gamma": 1.5}]
    for kw in bad:
        with pytest.raises(ValueError):
            opt.set_hparams(lr=5.0, **kw)
        assert torch.equal(opt._sched.sched, before), kw  # a rejected call changes nothing, its valid keys included
    opt.set_hparams(warmup_steps=2 ** 24 - 1, min_lr_ratio=1.0, lr_decay_gamma=1.0)
    with pytest.raises(ValueError):
        FusedAdamW(flat, lr_schedule="exponential")


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_clip_and_schedule_compose(kind):
    """clip_grad_norm_ + a per-step LR in torch.optim: the schedule is evaluated before the norm pass, clipping
    scales the gradient, the update uses the scheduled LR."""
    sched = SCHEDULES[0]
    net, flat, ref = _flat_net()
    x, y = _data(0)
    nn.functional.cross_entropy(net(x), y).backward()
    c = 0.3 * float(flat.grads.norm())
    flat.grads.zero_()
    opt = _make(kind, flat, max_grad_norm=c, lr_schedule="cosine")
    opt.set_hparams(**sched)
    groups = [{"params": [ref.fc.weight], "weight_decay": 0.1 if kind == "adamw" else 1e-2},
              {"params": [ref.fc.bias], "weight_decay": 0.0}]
    topt = (torch.optim.AdamW(groups, lr=1e-2, betas=(0.9, 0.95), eps=1e-8) if kind == "adamw"
            else torch.optim.SGD(groups, lr=0.05, momentum=0.9))
    clipped = 0
    for s in range(6):
        _step(opt, net, s)
        clipped += opt.clip_stats()["scale"] < 1.0
        assert float(opt.current_lr()) == _twin_lr(_base(kind), sched, s)
        for g in topt.param_groups:
            g["lr"] = _twin_lr(_base(kind), sched, s)
        x, y = _data(s)
        topt.zero_grad()
        nn.functional.cross_entropy(ref(x), y).backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), c)
        topt.step()
    assert clipped >= 1
    torch.testing.assert_close(flat.master("fc.weight"), ref.fc.weight.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(flat.master("fc.bias"), ref.fc.bias.detach(), rtol=1e-5, atol=1e-6)


def test_in_backward_updates_follow_the_schedule_bitwise():
    """FlatDDP(optimizer=opt) at world 1: the per-bucket updates inside the backward (``step_range_``) give bitwise
    the trajectory of the scheduled ``step_()`` after it; the schedule is evaluated once per step."""
    from polyaxon_amd.models.transformer import Transformer, lm_loss, tiny_llama
    from polyaxon_amd.ops import optim
    from polyaxon_amd.ops.flat import FlatParams
    from polyaxon_amd.parallel.ddp import FlatDDP

    sched = SCHEDULES[0]
    res = {}
    for in_bwd in (False, True):
        torch.manual_seed(0)
        model = Transformer(tiny_llama())
        flat = FlatParams(model, "cpu", channels_last=False)
        opt = optim.FusedAdamW(flat, lr=1e-2, weight_decay=0.1, lr_schedule="cosine")
        opt.set_hparams(**sched)
        ddp = FlatDDP(flat, bucket_mb=0.01, optimizer=opt if in_bwd else None)
        calls = []
        evaluate = opt._sched.evaluate
        opt._sched.evaluate = lambda *a, **k: (calls.append(1), evaluate(*a, **k))[1]
        gen = torch.Generator().manual_seed(9)
        lrs = []
        for s in range(5):
            tok = torch.randint(0, 256, (4, 16), generator=gen)
            lm_loss(model(tok), tok).backward()
            ddp.finish()
            opt.step_()
            opt.step += 1
            lrs.append(float(opt.current_lr()))
        assert len(calls) == 5
        if in_bwd:
            assert opt.in_backward and ddp.stepped > 5  # several buckets a step
        res[in_bwd] = (flat.params.clone(), lrs)
        ddp.close()
    assert torch.equal(res[False][0], res[True][0])
    assert res[False][1] == res[True][1] == [_twin_lr(1e-2, sched, s) for s in range(5)]


# ------------------------------------------------------------------ executor, programs, sweep
def _tiny_executor(**kw):
    from polyaxon_amd.polyflow.executor import ResidentTrialExecutor
    from polyaxon_amd.trainers import MLP

    g = torch.Generator().manual_seed(0)
    x = torch.randn(32, 784, generator=g)
    y = (x @ torch.randn(784, 10, generator=g)).argmax(1)
    return ResidentTrialExecutor(MLP(hidden=32), (x, y), "cpu", optimizer="sgd", channels_last=False, **kw)


def test_resume_continues_the_curve():
    """reset -> 3 steps -> snapshot -> 5 steps, against restore -> 5 steps: the step counter is the whole schedule
    state, so the restored trial repeats the same LRs and the same parameters."""
    sched = {"lr_schedule": "cosine", "warmup_steps": 2, "lr_total_steps": 8, "min_lr_ratio": 0.1}
    ex = _tiny_executor(lr_schedule=True)
    assert ex.opt.HP[-6:] == ("lr_schedule", "warmup_steps", "lr_total_steps", "min_lr_ratio", "lr_decay_gamma",
                              "lr_decay_every")
    ex.reset(seed=3)
    ex.set_hparams(lr=0.05, momentum=0.9, weight_decay=0.0, **sched)
    ex.run(3)
    assert float(ex.current_lr()) == _twin_lr(0.05, sched, 2)
    ex.snapshot("k")
    first = []
    for _ in range(5):
        ex.run(1)
        first.append(float(ex.current_lr()))
    p1 = ex.flat.params.clone()
    ex.restore("k")
    assert int(ex.step) == 3
    second = []
    for _ in range(5):
        ex.run(1)
        second.append(float(ex.current_lr()))
    assert first == second == [_twin_lr(0.05, sched, s) for s in range(3, 8)]
    assert torch.equal(ex.flat.params, p1)
    plain = _tiny_executor()
    assert "warmup_steps" not in plain.opt.HP


@pytest.mark.parametrize("name", ["resnet_tiny", "gpt2_tiny"])
def test_programs_schedule_per_trial(name):
    from polyaxon_amd.ops import lr_schedule as lrs
    from polyaxon_amd.polyflow.programs import build_program, lr_horizon

    plain = build_program(name, {}, "cpu")
    assert not any(k in plain.hp_keys for k in lrs.KEYS) and lr_horizon(plain) is None
    assert "lr_schedule" not in plain.info["warm_hparams"]
    prog = build_program(name, {"lr_schedule": True, "clip_grad": True}, "cpu")
    assert prog.hp_keys == plain.hp_keys + ("max_grad_norm",) + lrs.KEYS
    assert prog.info["warm_hparams"]["lr_schedule"] == "cosine" and prog.info["warm_hparams"]["warmup_steps"] > 0
    assert prog.info["lr_schedule"] == "constant" and lr_horizon(prog) == "max"
    assert lr_horizon(build_program(name, {"lr_schedule": "linear", "lr_horizon": "rung"}, "cpu")) == "rung"
    with pytest.raises(ValueError):
        build_program(name, {"lr_schedule": "cosine", "lr_horizon": "bracket"}, "cpu")
    with pytest.raises(ValueError):
        build_program(name, {"lr_schedule": "exponential"}, "cpu")
    prog = build_program(name, {"lr_schedule": "cosine"}, "cpu")
    prog.warm(steps=1)
    ex = prog.executor
    assert ex.opt._sched.sched.tolist()[1:4] == [2.0, 0.0, 0.0]  # warm() left the program's kind, not its own
    base = prog.info["warm_hparams"]["lr"]
    curves = {}
    for trial in ({"warmup_steps": 1, "min_lr_ratio": 0.5}, {"warmup_steps": 3, "min_lr_ratio": 0.0}):
        ex.reset(seed=1)
        hp = dict(prog.info["warm_hparams"], lr_schedule="cosine", lr_total_steps=5, **trial)
        ex.set_hparams(**{k: v for k, v in hp.items() if k in prog.hp_keys})
        lr = []
        for _ in range(5):
            ex.run(1)
            lr.append(float(ex.current_lr()))
        assert lr == [_twin_lr(base, hp, s) for s in range(5)]
        curves[trial["warmup_steps"]] = lr
    assert curves[1] != curves[3] and curves[1][0] == pytest.approx(base) and curves[3][0] == pytest.approx(base / 3)


class _SpyExecutor:
    """Records what a sweep driver sets; everything else is the real executor."""

    def __init__(self, ex):
        self._ex = ex
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._ex, name)

    def set_hparams(self, **hp):
        self.calls.append(dict(hp))
        self._ex.set_hparams(**hp)


def _hyperband(resume=True):
    from polyaxon_amd.polytune.managers import HyperbandSearchManager
    from polyaxon_amd.spec.hptuning import HPTuningConfig

    cfg = {"seed": 1, "concurrency": 1,
           "hyperband": {"max_iter": 9, "eta": 3, "resource": {"name": "units", "type": "int"},
                         "metric": {"name": "loss", "optimization": "minimize"}, "resume": resume},
           "matrix": {"lr": {"loguniform": [-5, -2]}, "warmup_steps": {"values": [0, 2]}}}
    return HyperbandSearchManager(HPTuningConfig.from_dict(cfg))


@pytest.mark.parametrize("mode", ["max", "rung"])
def test_hyperband_sweep_supplies_the_horizon(mode):
    from polyaxon_amd.polyflow.sweep import HyperbandSweep

    unit_steps = 2
    ex = _SpyExecutor(_tiny_executor(lr_schedule="cosine"))
    sweep = HyperbandSweep(_hyperband(), ex, unit_steps=unit_steps, lr_horizon=mode)
    res = sweep.run(max_trials=12)
    assert len(ex.calls) == len(res.trials) == 12
    rungs = set()
    for rec, hp in zip(res.trials, ex.calls):
        want = 9 * unit_steps if mode == "max" else int(round(rec.resource * unit_steps))
        assert hp["lr_total_steps"] == want, (rec, hp)
        assert "warmup_steps" in hp and "units" not in hp
        rungs.add(rec.resource)
    assert len(rungs) > 1  # more than one rung ran: `rung` horizons differ, `max` ones do not
    # a trial that names its own horizon keeps it; an executor without a schedule gets no horizon
    from polyaxon_amd.ops import lr_schedule as lrs

    assert lrs.with_horizon({"lr": 0.1, "lr_total_steps": 7}, mode, 9, 3, 2)["lr_total_steps"] == 7
    assert lrs.with_horizon({"lr": 0.1}, None, 9, 3, 2) == {"lr": 0.1}
    plain = _SpyExecutor(_tiny_executor())
    HyperbandSweep(_hyperband(), plain, unit_steps=unit_steps, lr_horizon=mode).run(max_trials=2)
    assert all("lr_total_steps" not in hp for hp in plain.calls)
    with pytest.raises(ValueError):
        HyperbandSweep(_hyperband(), ex, unit_steps=unit_steps, lr_horizon="bracket")


def test_resident_worker_supplies_the_horizon():
    """The resident worker's bracket, ASHA and fixed-budget (BO) paths share the rule (``_trial_hparams``)."""
    from polyaxon_amd.polyflow.resident import ResidentWorker, _FixedBudget

    w = ResidentWorker("resnet_tiny", {"lr_schedule": "cosine", "unit_steps": 3}, device="cpu")
    w.build()
    assert w._trial_hparams({"lr": 0.1, "warmup_steps": 2, "units": 3, "junk": 1}, 9, 3) == {
        "lr": 0.1, "warmup_steps": 2, "lr_total_steps": 27}
    assert w._trial_hparams({"lr": 0.1, "lr_total_steps": 5}, 9, 3)["lr_total_steps"] == 5
    fb = _FixedBudget(4.0)  # a BO trial: the horizon is its own step count
    r = fb.get_n_resources_for_iteration(0, 0)
    assert w._trial_hparams({"lr": 0.1}, fb.max_iter, r)["lr_total_steps"] == 12
    w2 = ResidentWorker("resnet_tiny", {"lr_schedule": "cosine", "lr_horizon": "rung", "unit_steps": 3}, device="cpu")
    w2.build()
    assert w2._trial_hparams({"lr": 0.1}, 9, 3)["lr_total_steps"] == 9
    w3 = ResidentWorker("resnet_tiny", {"unit_steps": 3}, device="cpu")
    w3.build()
    assert w3._trial_hparams({"lr": 0.1, "warmup_steps": 2}, 9, 3) == {"lr": 0.1}


# ------------------------------------------------------------------ trainers, example
class _Tracker:
    def __init__(self):
        self.rows = []

    def log_metrics(self, step=None, **metrics):
        self.rows.append((step, {k: float(v) for k, v in metrics.items()}))

    def close(self):
        pass


def _clean_env(monkeypatch):
    for k in ("PLX_ZERO1", "PLX_OPT_IN_BACKWARD", "POLYAXON_DECLARATIONS"):
        monkeypatch.delenv(k, raising=False)


def test_lm_trainer_follows_the_schedule(capsys, monkeypatch):
    from polyaxon_amd import trainers

    _clean_env(monkeypatch)
    xp = _Tracker()
    monkeypatch.setattr(trainers, "_tracker", lambda: xp)
    sets = []
    from polyaxon_amd.ops.optim import FusedAdamW

    orig = FusedAdamW.set_hparams
    monkeypatch.setattr(FusedAdamW, "set_hparams", lambda self, **hp: (sets.append(hp), orig(self, **hp))[1])
    loss = trainers.train_lm(["--cpu", "--model", "tiny", "--steps", "6", "--log_every", "1", "--lr", "0.01",
                              "--lr_schedule", "cosine", "--warmup_steps", "2", "--min_lr_ratio", "0.1"])
    assert math.isfinite(loss)
    sched = {"lr_schedule": "cosine", "warmup_steps": 2, "lr_total_steps": 6, "min_lr_ratio": 0.1}
    logged = [(step, row["lr"]) for step, row in xp.rows if "lr" in row and "tokens_per_s" not in row]
    assert logged == [(it + 1, _twin_lr(0.01, sched, it)) for it in range(6)]
    assert len(sets) == 2  # the constructor's and the schedule's: no per-step set_hparams
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["lr"] == _twin_lr(0.01, sched, 5)
    # off (the default): the host-side warm-up path is what it was -- one set_hparams per step, no lr in the output
    sets.clear()
    xp.rows.clear()
    trainers.train_lm(["--cpu", "--model", "tiny", "--steps", "3", "--log_every", "1", "--warmup_steps", "2"])
    assert len(sets) == 1 + 3 and [round(s["lr"], 9) for s in sets[1:]] == [0.0005, 0.001, 0.001]
    assert all("lr" not in row for _, row in xp.rows)
    assert "lr" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_resnet_trainer_follows_the_schedule(capsys, monkeypatch):
    from polyaxon_amd import trainers

    _clean_env(monkeypatch)
    xp = _Tracker()
    monkeypatch.setattr(trainers, "_tracker", lambda: xp)
    args = ["--cpu", "--bs", "2", "--image", "32", "--units", "2", "--unit_steps", "2", "--lr", "0.05"]
    trainers.train_resnet(args + ["--lr_schedule", "cosine", "--warmup_steps", "2", "--min_lr_ratio", "0.1"])
    sched = {"lr_schedule": "cosine", "warmup_steps": 2, "lr_total_steps": 4, "min_lr_ratio": 0.1}
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["lr"] == _twin_lr(0.05, sched, 3)
    assert xp.rows[-1][0] == 4 and xp.rows[-1][1]["lr"] == out["lr"]
    xp.rows.clear()
    trainers.train_resnet(args)
    assert "lr" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "lr" not in xp.rows[-1][1]


def test_example_file_searches_schedule_keys():
    import os

    import yaml

    from polyaxon_amd.ops import lr_schedule as lrs
    from polyaxon_amd.polyflow.programs import PROGRAMS, build_program

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "gpt2_bo_sched.yml")
    with open(path) as f:
        spec = yaml.safe_load(f)
    ex = spec["environment"]["executor"]
    assert ex["kind"] == "resident" and ex["program"] == "gpt2" and ex["program"] in PROGRAMS
    assert ex["params"]["lr_schedule"] == "cosine"
    matrix = spec["hptuning"]["matrix"]
    assert {"lr", "warmup_steps", "min_lr_ratio"} <= set(matrix)
    # the same builder at CPU-test size understands every searched key
    params = {k: v for k, v in ex["params"].items() if k in ("lr_schedule", "lr_horizon")}
    prog = build_program("gpt2_tiny", params, "cpu")
    assert set(matrix) <= set(prog.hp_keys) and set(lrs.KEYS) <= set(prog.hp_keys)
    from polyaxon_amd.spec import specification_for

    with open(path) as f:
        assert specification_for(f.read()).kind == "group"
