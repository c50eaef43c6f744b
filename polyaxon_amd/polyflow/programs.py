"""Trial programs for resident executors: what a warm worker builds once and then trains trial after trial.

A *program* is the trial-invariant part of an experiment -- model architecture, batch shape, data stream,
optimizer kind, the step (eager or captured as a hipGraph) -- and is named in the Polyaxonfile as
``environment.executor: {kind: resident, program: <name>, params: {...}}``.  Everything that varies between
trials (hyper-parameters, random init seed, Hyperband resource) is device data the executor rewrites in place
(polyflow/executor.py).  In the reference every trial is a pod running ``run.cmd`` from scratch
(polyaxon/scheduler/spawners/experiment_spawner.py:108-179); the program is what stays warm instead.

Registry: ``resnet50`` (BASELINE.json config 3), ``resnet_tiny`` (same code path, CPU-test sized), ``mlp``
(config 2), ``gpt2`` (config 4's GPT-2 125M trial), ``gpt2_tiny`` (same code path, CPU-test sized).  ``module:callable`` names any user factory with the same signature ``(params, device) -> TrialProgram``.

Every built-in program takes ``params: {clip_grad: true}``: global-norm gradient clipping in the step, with
``max_grad_norm`` as one more per-trial hyper-parameter (device data like the rest; 0 = no limit).

Every built-in program also takes ``params: {lr_schedule: true | <kind>}``: the device-resident LR schedule
(ops/optim.py) with ``lr_schedule`` (constant, linear, cosine, step, inv_sqrt), ``warmup_steps``, ``lr_total_steps``,
``min_lr_ratio``, ``lr_decay_gamma`` and ``lr_decay_every`` as per-trial hyper-parameters and ``lr`` as the base LR;
``true`` starts every trial at ``constant``.  A trial that names no ``lr_total_steps`` gets the horizon from the
sweep driver (``params: {lr_horizon: max | rung}``, default ``max``; ops/lr_schedule.py horizon_steps).

Every built-in program also takes ``params: {loss_hparams: true}``: ``label_smoothing`` and ``z_loss`` as per-trial
hyper-parameters of the loss (ops/loss_hp.py), read from device memory by the fused cross-entropy kernels, both 0
until a trial sets them.  The metric the program commits is then the plain NLL, not the training loss, so trials
with different smoothing stay comparable.

``gpt2`` and ``gpt2_tiny`` also take ``params: {dropout: true, dropout_seed: n}``: residual and embedding dropout
(ops/dropout.py) with the rate ``dropout`` as a per-trial hyper-parameter, 0 until a trial sets it.  The rate is
device data and no mask is stored: the step's kernels draw it from the device step counter, so one captured step
serves every rate and draws fresh masks every replay.  ``dropout_seed`` keys the masks for the whole program, so
trials differ by their weights and rates, not by their masks.  The other programs have no dropout sites and reject it.

``gpt2`` and ``gpt2_tiny`` also take ``params: {attn_dropout: true}``: dropout on the attention probabilities
(ops/attn_dropout.py, drawn inside the flash-attention kernels) with the rate ``attn_dropout`` as a per-trial
hyper-parameter, 0 until a trial sets it.  It is independent of ``dropout`` -- either or both may be on -- and shares
``dropout_seed``.  The other programs reject it.
"""
from __future__ import annotations

import functools
import importlib
import math
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Optional, Tuple

# torch is imported inside the builders: the scheduler imports this module for program_key / bracket_units, and the
# scheduler process never loads torch or the HIP runtime (tests/test_gpu_free_scheduler.py)


@dataclass
class TrialProgram:
    executor: Any                     # ResidentTrialExecutor
    unit_steps: int = 1               # training steps per Hyperband / ASHA resource unit
    metric: str = "loss"              # the metric the executor commits (mean loss over the last `window` steps)
    window: int = 4
    hp_keys: Tuple[str, ...] = ()     # hyper-parameters the program understands
    info: Dict[str, Any] = field(default_factory=dict)

    def warm(self, steps: int = 2) -> None:
        """Pay one-time costs (kernel selection, allocator growth, library page-in) before the first trial."""
        import torch

        ex = self.executor
        if ex.use_graph:
            ex.capture(warmup=steps)
        else:
            ex.reset(seed=0)
            ex.set_hparams(**{k: v for k, v in self.info.get("warm_hparams", {}).items()})
            ex.run(steps)
            ex.snapshot("__warm__")
            ex.restore("__warm__")
            ex.drop("__warm__")
            if self.info.get("lr_schedule"):  # back from the warm-up's schedule to the program's own kind
                from polyaxon_amd.ops import lr_schedule as lrs

                ex.set_hparams(**dict(lrs.DEFAULTS, lr_schedule=self.info["lr_schedule"]))
            if self.info.get("loss_hparams"):  # back from the warm-up's smoothing and z-loss to none
                from polyaxon_amd.ops import loss_hp

                ex.set_hparams(**loss_hp.DEFAULTS)
            if self.info.get("dropout"):  # back from the warm-up's rate to none
                from polyaxon_amd.ops import dropout

                ex.set_hparams(**dropout.DEFAULTS)
            if self.info.get("attn_dropout"):
                from polyaxon_amd.ops import attn_dropout

                ex.set_hparams(**attn_dropout.DEFAULTS)
        if ex.is_cuda:
            torch.cuda.synchronize(ex.device)


def _clip_grad(params: Dict[str, Any]) -> bool:
    return bool(params.get("clip_grad", False))


def _with_clip(prog: TrialProgram, clip: bool) -> TrialProgram:
    """``clip_grad`` programs understand ``max_grad_norm`` and warm up with a limit set."""
    if clip:
        prog.hp_keys = prog.hp_keys + ("max_grad_norm",)
        prog.info["warm_hparams"] = {**prog.info.get("warm_hparams", {}), "max_grad_norm": 1.0}
        prog.info["clip_grad"] = True
    return prog


def _loss_hparams(params: Dict[str, Any]) -> bool:
    return bool(params.get("loss_hparams", False))


def _with_loss_hp(prog: TrialProgram, on: bool) -> TrialProgram:
    """``loss_hparams`` programs understand ``label_smoothing`` and ``z_loss`` and warm up with both set, so the
    warm steps run the full path."""
    if on:
        from polyaxon_amd.ops import loss_hp

        prog.hp_keys = prog.hp_keys + loss_hp.KEYS
        prog.info["warm_hparams"] = {**prog.info.get("warm_hparams", {}), "label_smoothing": 0.1, "z_loss": 1e-4}
        prog.info["loss_hparams"] = True
    return prog


def _dropout(params: Dict[str, Any]) -> bool:
    return bool(params.get("dropout", False))


def _attn_dropout(params: Dict[str, Any]) -> bool:
    return bool(params.get("attn_dropout", False))


def _no_dropout(name: str, params: Dict[str, Any]) -> None:
    if _dropout(params) or "dropout_seed" in params:
        raise ValueError(f"program {name} has no dropout sites: `dropout` is a param of gpt2 / gpt2_tiny only")
    if _attn_dropout(params):
        raise ValueError(f"program {name} has no attention: `attn_dropout` is a param of gpt2 / gpt2_tiny only")


def _with_attn_dropout(prog: TrialProgram, on: bool) -> TrialProgram:
    """``attn_dropout`` programs understand the ``attn_dropout`` rate and warm up at 0.1, so the warm steps draw
    masks."""
    if on:
        from polyaxon_amd.ops import attn_dropout

        prog.hp_keys = prog.hp_keys + attn_dropout.KEYS
        prog.info["warm_hparams"] = {**prog.info.get("warm_hparams", {}), "attn_dropout": 0.1}
        prog.info["attn_dropout"] = True
    return prog


def _with_dropout(prog: TrialProgram, on: bool) -> TrialProgram:
    """``dropout`` programs understand the ``dropout`` rate and warm up at 0.1, so the warm steps draw masks."""
    if on:
        from polyaxon_amd.ops import dropout

        prog.hp_keys = prog.hp_keys + dropout.KEYS
        prog.info["warm_hparams"] = {**prog.info.get("warm_hparams", {}), "dropout": 0.1}
        prog.info["dropout"] = True
    return prog


def _lr_schedule(params: Dict[str, Any]):
    """The program's ``lr_schedule`` param as the executor takes it: False, or a kind name (true = constant)."""
    from polyaxon_amd.ops import lr_schedule as lrs

    v = params.get("lr_schedule", False)
    if v is None or v is False:
        return False
    return "constant" if v is True else lrs.KINDS[lrs.kind_code(v)]


def _with_schedule(prog: TrialProgram, params: Dict[str, Any]) -> TrialProgram:
    """``lr_schedule`` programs understand the schedule's keys, warm up on a cosine schedule with warm-up (so the
    warm steps run the kernel's longest path) and tell the sweep driver which horizon a trial without
    ``lr_total_steps`` gets (``info["lr_horizon"]``)."""
    from polyaxon_amd.ops import lr_schedule as lrs

    kind = _lr_schedule(params)
    if kind:
        mode = str(params.get("lr_horizon", "max"))
        lrs.horizon_steps(mode, 1, 1, 1)  # rejects an unknown mode when the program is built
        prog.hp_keys = prog.hp_keys + lrs.KEYS
        prog.info["warm_hparams"] = {**prog.info.get("warm_hparams", {}), "lr_schedule": "cosine", "warmup_steps": 1,
                                     "lr_total_steps": 4, "min_lr_ratio": 0.1}
        prog.info["lr_schedule"] = kind
        prog.info["lr_horizon"] = mode
    return prog


def lr_horizon(prog) -> Optional[str]:
    """The program's ``lr_horizon`` mode when it has a schedule, else None (ops/lr_schedule.py with_horizon)."""
    return (getattr(prog, "info", None) or {}).get("lr_horizon")


def _resnet(params: Dict[str, Any], device, tiny: bool) -> TrialProgram:
    import torch

    from polyaxon_amd.models.resnet import resnet18ish, resnet50
    from polyaxon_amd.ops.synth import SyntheticImages
    from polyaxon_amd.polyflow.executor import ResidentTrialExecutor

    _no_dropout("resnet_tiny" if tiny else "resnet50", params)
    dev = torch.device(device)
    batch = int(params.get("batch", 8 if tiny else 256))
    image = int(params.get("image", 32 if tiny else 224))
    classes = int(params.get("classes", 10 if tiny else 1000))
    data = SyntheticImages(batch, image, dev, classes=classes,
                           active_classes=int(params.get("active_classes", min(classes, 100))),
                           grid=int(params.get("grid", 4 if tiny else 7)), signal=float(params.get("signal", 0.5)),
                           seed=int(params.get("data_seed", 0)))
    model = resnet18ish(num_classes=classes) if tiny else resnet50(num_classes=classes)
    clip = _clip_grad(params)
    ex = ResidentTrialExecutor(model, data, dev, optimizer="sgd", use_graph=bool(params.get("graph", False)),
                               clip_grad=clip, lr_schedule=_lr_schedule(params), loss_hparams=_loss_hparams(params))
    return _with_loss_hp(_with_schedule(_with_clip(TrialProgram(
        ex, unit_steps=int(params.get("unit_steps", 1 if tiny else 4)),
        window=int(params.get("window", 4)), hp_keys=("lr", "momentum", "weight_decay", "nesterov"),
        info={"model": "resnet18ish" if tiny else "resnet50", "batch": batch, "image": image,
              "classes": classes, "data": "synthetic, fresh per step (ops/synth.py)",
              "warm_hparams": {"lr": 0.01, "momentum": 0.9, "weight_decay": 1e-4},
              "images_per_step": batch}), clip), params), _loss_hparams(params))


def _mlp(params: Dict[str, Any], device) -> TrialProgram:
    import torch

    from polyaxon_amd.polyflow.executor import ResidentTrialExecutor
    from polyaxon_amd.trainers import MLP

    _no_dropout("mlp", params)
    dev = torch.device(device)
    bs = int(params.get("batch", 256))
    g = torch.Generator().manual_seed(int(params.get("data_seed", 0)))
    x = torch.randn(bs, 784, generator=g)
    y = (x @ torch.randn(784, 10, generator=g)).argmax(1)
    clip = _clip_grad(params)
    ex = ResidentTrialExecutor(MLP(), (x, y), dev, optimizer="sgd", use_graph=dev.type == "cuda", channels_last=False,
                               clip_grad=clip, lr_schedule=_lr_schedule(params), loss_hparams=_loss_hparams(params))
    return _with_loss_hp(_with_schedule(_with_clip(TrialProgram(
        ex, unit_steps=int(params.get("unit_steps", 10)), window=int(params.get("window", 4)),
        hp_keys=("lr", "momentum", "weight_decay"),
        info={"model": "mlp", "batch": bs, "warm_hparams": {"lr": 0.01, "momentum": 0.9},
              "images_per_step": bs}), clip), params), _loss_hparams(params))


def _gpt2(params: Dict[str, Any], device, tiny: bool) -> TrialProgram:
    import torch

    """GPT-2 125M (BASELINE.json config 4's trial) on the synthetic copy-task token stream (ops/synth.py
    SyntheticTokens): bf16 weights / gradients with an fp32 master and fused AdamW (the LM trainer's numerics),
    every trial re-initialised in place (GPT-2 init via plx_init_flat), AdamW hyper-parameters as device data."""
    from polyaxon_amd.models.transformer import Transformer, gpt2_125m, lm_loss
    from polyaxon_amd.ops.synth import SyntheticChain, SyntheticTokens
    from polyaxon_amd.polyflow.executor import ResidentTrialExecutor

    dev = torch.device(device)
    if tiny:
        # heads: 1 gives head_dim 64, the smallest the flash-attention kernels take (2: the fp32 math fallback)
        cfg = gpt2_125m(vocab_size=int(params.get("vocab", 256)), n_layers=2, d_model=64,
                        n_heads=int(params.get("heads", 2)), d_ff=256, max_seq_len=int(params.get("seq", 32)))
    else:
        cfg = gpt2_125m(vocab_size=int(params.get("vocab", 50257)))
    batch = int(params.get("batch", 2 if tiny else 16))
    seq = int(params.get("seq", 32 if tiny else 1024))
    task = str(params.get("task", "copy"))
    if task == "chain":  # a memorised transition table: learning-rate sensitive within ~100 steps
        data = SyntheticChain(batch, seq, cfg.vocab_size, dev, p=int(params.get("chain_p", 251 if tiny else 4093)),
                              seed=int(params.get("data_seed", 0)))
    else:
        data = SyntheticTokens(batch, seq, cfg.vocab_size, dev, period=int(params.get("period", 8 if tiny else 64)),
                               seed=int(params.get("data_seed", 0)), active_vocab=int(params.get("active_vocab", 0)))
    if dev.type == "cuda":
        with torch.device(dev):
            model = Transformer(cfg)
    else:
        model = Transformer(cfg)
    clip = _clip_grad(params)
    loss_hp = _loss_hparams(params)
    # the smoothing term runs over the real vocabulary, not the -inf padding columns of the padded head
    loss_fn = functools.partial(lm_loss, n_classes=cfg.vocab_size) if loss_hp else lm_loss
    ex = ResidentTrialExecutor(model, data, dev, loss_fn=loss_fn, optimizer="adamw",
                               use_graph=bool(params.get("graph", False)), channels_last=False,
                               lp_dtype=torch.bfloat16, clip_grad=clip, lr_schedule=_lr_schedule(params),
                               loss_hparams=loss_hp, dropout=_dropout(params),
                               dropout_seed=int(params.get("dropout_seed", 0)), attn_dropout=_attn_dropout(params))
    return _with_attn_dropout(_with_dropout(_with_loss_hp(_with_schedule(_with_clip(TrialProgram(
        ex, unit_steps=int(params.get("unit_steps", 4 if tiny else 10)),
        window=int(params.get("window", 4)),
        hp_keys=("lr", "beta1", "beta2", "eps", "weight_decay"),
        info={"model": "gpt2_tiny" if tiny else "gpt2_125m", "batch": batch, "seq": seq,
              "vocab": cfg.vocab_size, "data": f"synthetic {task} task, fresh per step (ops/synth.py)",
              "warm_hparams": {"lr": 3e-4, "beta1": 0.9, "beta2": 0.95, "eps": 1e-8,
                               "weight_decay": 0.1},
              "tokens_per_step": batch * seq, "floor_loss": data.floor_loss,
              "unigram_loss": data.unigram_loss, "chance_loss": data.chance_loss,
              "active_vocab": data.active_vocab}), clip), params), loss_hp), _dropout(params)), _attn_dropout(params))


PROGRAMS: Dict[str, Callable[[Dict[str, Any], Any], TrialProgram]] = {
    "gpt2": lambda p, d: _gpt2(p, d, tiny=False),
    "gpt2_tiny": lambda p, d: _gpt2(p, d, tiny=True),
    "resnet50": lambda p, d: _resnet(p, d, tiny=False),
    "resnet_tiny": lambda p, d: _resnet(p, d, tiny=True),
    "mlp": _mlp,
}


def resolve(name: str) -> Callable[[Dict[str, Any], Any], TrialProgram]:
    if name in PROGRAMS:
        return PROGRAMS[name]
    if ":" in name:
        mod, _, attr = name.partition(":")
        return getattr(importlib.import_module(mod), attr)
    raise KeyError(f"unknown resident program {name!r}; known: {sorted(PROGRAMS)} or module:callable")


def build_program(name: str, params: Optional[Dict[str, Any]], device) -> TrialProgram:
    prog = resolve(name)(dict(params or {}), device)
    if not isinstance(prog, TrialProgram):
        raise TypeError(f"program {name} returned {type(prog).__name__}, expected TrialProgram")
    return prog


def program_key(name: str, params: Optional[Dict[str, Any]]) -> str:
    """Executors are shared by every group whose program (name + build params) is identical."""
    import json

    return f"{name}:{json.dumps(params or {}, sort_keys=True)}"


def bracket_units(max_iter: float, eta: float, iteration: int, resume: bool) -> float:
    """Training resource (in units) one Hyperband bracket costs -- the load the pool balances across executors."""
    s_max = int(math.log(max_iter) / math.log(eta))
    s = s_max - iteration
    B = (s_max + 1) * max_iter
    n0 = int(math.ceil((B / max_iter) * (eta ** s) / (s + 1)))
    r = max_iter * eta ** (-s)
    total, prev, n, i = 0.0, 0.0, n0, 0
    while n > 0:
        ri = r * eta ** i
        total += n * ((ri - prev) if (resume and i) else ri)
        prev = ri
        # the reference's create_iteration: a bracket with a successor ends at rung s (should_reschedule); the last
        # bracket (s = 0) takes one more reduction, keep = int(n0 / eta) (the reference quirk), and none after it
        # (get_n_config_to_keep_for_iteration is 0 at rung s + 1)
        n = 0 if (i >= s and iteration < s_max) or i == s + 1 else int(n0 * (eta ** -i) / eta)
        i += 1
    return total


def asha_units(n_configs: int, min_r: float, max_r: float, eta: float, resume: bool) -> float:
    """Expected training resource (in units) of an ASHA shard over ``n_configs`` configs: rung k holds about
    n / eta^k configs, each training r_k (or r_k - r_{k-1} when resumed) -- the load the pool balances."""
    n_rungs = int(math.floor(math.log(max_r / min_r) / math.log(eta) + 1e-9)) + 1
    total, prev = 0.0, 0.0
    for k in range(n_rungs):
        rk = min(min_r * eta ** k, max_r)
        total += (n_configs / eta ** k) * ((rk - prev) if (resume and k) else rk)
        prev = rk
    return total
