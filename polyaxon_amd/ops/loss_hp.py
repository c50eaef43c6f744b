"""Device-resident hyper-parameters of the loss: label smoothing and z-loss (ops/lm.py ``loss_hp=``).

Names, defaults and validation are pure Python on purpose: polyflow/programs.py reads the key names from here, and
the scheduler process that imports it never loads torch (tests/test_gpu_free_scheduler.py).  :class:`LossHParams`
imports torch when it is built.  The formulas live in the ``plx_xent_hp_*`` kernels (csrc/lm_kernels.hip) and in the
torch fallback of ops/lm.py:

    nll  = lse - x[t]
    loss = lse - (1 - eps) x[t] - eps mean_{j<C} x[j] + zeta lse^2

with eps = ``label_smoothing``, zeta = ``z_loss`` and C the number of real classes.
"""
from __future__ import annotations

import math
from typing import Any, Dict

KEYS = ("label_smoothing", "z_loss")  # slots 0 and 1 of the 4-float device tensor; 2 and 3 are reserved (0)

DEFAULTS: Dict[str, float] = {"label_smoothing": 0.0, "z_loss": 0.0}


def validate(key: str, value: Any) -> float:
    """The fp32 slot value of loss hyper-parameter ``key``; ValueError when it is outside its domain."""
    if key not in KEYS:
        raise KeyError(key)
    v = float(value)
    if not math.isfinite(v):
        raise ValueError(f"{key} must be finite, got {value!r}")
    if key == "label_smoothing":
        if not 0.0 <= v < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {value!r}")
    elif v < 0.0:
        raise ValueError(f"z_loss must be >= 0, got {value!r}")
    return v


class LossHParams:
    """What a loss with per-trial hyper-parameters reads and writes on ``device``:

    ``hp``   4 fp32 -- [0] ``label_smoothing``, [1] ``z_loss``, [2], [3] reserved (0) -- that the fused cross-entropy
             kernels read at run time, so one captured step serves every value;
    ``nll``  a 0-dim fp32 tensor the fused ops overwrite every forward with the step's mean plain negative
             log-likelihood (the averaging rule of the loss itself): the metric that stays comparable between
             trials whose training losses differ by their own smoothing.

    Both are allocated here, never during a capture.  ``set`` is one 16-byte copy through a pinned staging ring (a
    plain copy on the CPU); ``host`` is the copy the torch fallback reads instead of the device."""

    def __init__(self, device):
        import torch

        self.device = torch.device(device)
        self.hp = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.nll = torch.zeros((), dtype=torch.float32, device=self.device)
        self.host: Dict[str, float] = dict(DEFAULTS)
        self._ring = None
        if self.device.type == "cuda":
            from polyaxon_amd.ops.optim import _PinnedRing

            self._ring = _PinnedRing(width=4)

    def set(self, **kv) -> None:
        """Validate, merge into the host copy and upload; a rejected call changes nothing."""
        import torch

        new = {k: validate(k, v) for k, v in kv.items()}
        self.host.update(new)  # only once every value has passed
        values = [self.host[k] for k in KEYS] + [0.0, 0.0]
        if self._ring is None:
            self.hp.copy_(torch.tensor(values, dtype=torch.float32))
        else:
            self._ring.copy_to(self.hp, values)

    @property
    def label_smoothing(self) -> float:
        return self.host["label_smoothing"]

    @property
    def z_loss(self) -> float:
        return self.host["z_loss"]
