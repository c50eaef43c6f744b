"""Names, defaults and validation of the device-resident learning-rate schedule (ops/optim.py ``lr_schedule=``).

Pure Python on purpose: polyflow/programs.py reads the key names and the horizon rule from here, and the scheduler
process that imports it never loads torch (tests/test_gpu_free_scheduler.py).  The formula itself lives in
``plx_lr_schedule`` (csrc/train_kernels.hip) and its torch float32 twin ``ops.optim.lr_factor``.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

KINDS = ("constant", "linear", "cosine", "step", "inv_sqrt")  # the kind code is the index

# the hyper-parameters a scheduled optimizer gains, in `sched` slot order 1..6 (slot 0 is `lr`, the base LR)
KEYS = ("lr_schedule", "warmup_steps", "lr_total_steps", "min_lr_ratio", "lr_decay_gamma", "lr_decay_every")

DEFAULTS: Dict[str, float] = {"lr_schedule": 0.0, "warmup_steps": 0.0, "lr_total_steps": 0.0, "min_lr_ratio": 0.0,
                              "lr_decay_gamma": 0.1, "lr_decay_every": 1.0}

MAX_STEPS = 1 << 24  # steps travel as fp32: exact below 2^24


def kind_code(kind: Any) -> int:
    """The code of a kind given as a name or as a code (int, or a float holding one)."""
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"unknown lr_schedule {kind!r}; known: {', '.join(KINDS)}")
        return KINDS.index(kind)
    if isinstance(kind, bool) or not isinstance(kind, (int, float)) or int(kind) != kind \
            or not 0 <= int(kind) < len(KINDS):
        raise ValueError(f"unknown lr_schedule {kind!r}; known: {', '.join(KINDS)} or their codes 0..{len(KINDS) - 1}")
    return int(kind)


def validate(key: str, value: Any) -> float:
    """The fp32 slot value of schedule hyper-parameter ``key``; ValueError when it is outside its domain."""
    if key == "lr_schedule":
        return float(kind_code(value))
    v = float(value)
    if key in ("warmup_steps", "lr_total_steps", "lr_decay_every"):
        if not (0 <= v < MAX_STEPS) or v != int(v):
            raise ValueError(f"{key} must be a whole number of steps in [0, 2^24), got {value!r}")
    elif key == "min_lr_ratio":
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"min_lr_ratio must be in [0, 1], got {value!r}")
    elif key == "lr_decay_gamma":
        if not 0.0 < v <= 1.0:
            raise ValueError(f"lr_decay_gamma must be in (0, 1], got {value!r}")
    else:
        raise KeyError(key)
    return v


def horizon_steps(mode: str, max_resource: float, resource: float, unit_steps: int) -> int:
    """``lr_total_steps`` a sweep driver supplies to a trial that names none.

    ``max``: ``max_resource x unit_steps`` -- every trial of a bracket or shard shares one curve, and a promotion
    that resumes from its snapshot continues along it.  ``rung``: this rung's cumulative ``resource x unit_steps`` --
    each rung anneals fully; a promotion that resumes is then a warm restart: its step counter continues, so the
    LR jumps from the last rung's floor back up to where the longer curve stands at that step."""
    if mode not in ("max", "rung"):
        raise ValueError(f"lr_horizon must be 'max' or 'rung', got {mode!r}")
    return int(round((max_resource if mode == "max" else resource) * unit_steps))


def with_horizon(params: Dict[str, Any], mode: Optional[str], max_resource: float, resource: float,
                 unit_steps: int) -> Dict[str, Any]:
    """``params`` with ``lr_total_steps`` filled in by :func:`horizon_steps` -- when the program has a schedule
    (``mode`` is its ``lr_horizon``; None: no schedule) and the trial's own params carry none."""
    if mode is None or "lr_total_steps" in params:
        return params
    return dict(params, lr_total_steps=horizon_steps(mode, max_resource, resource, unit_steps))
