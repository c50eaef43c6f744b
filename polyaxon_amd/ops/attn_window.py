"""Sliding-window (local, Mistral-style) attention as a device-resident hyper-parameter: query ``i`` sees key ``j``
iff ``i - W < j <= i`` -- the last ``W`` keys counting itself.  ``W`` is one int32 of device memory that the windowed
flash-attention kernels (csrc/attn_kernels.hip ``plx_attn_win_fwd`` / ``plx_attn_win_bwd``) load at run time, so one
captured step serves every window of a sweep and a trial changes it with one 4-byte copy.

``attn_window = 0`` means no window: plain causal attention, bit for bit.  Windowed attention is causal
self-attention only (``S == Skv``), so every query keeps its diagonal key and no row is ever fully masked.  Unlike
dropout the window is part of the model: it holds in ``eval()`` and in activation-checkpoint recomputation alike.

Names, defaults and validation are pure Python on purpose: polyflow/programs.py reads the key names from here, and
the scheduler process that imports it never loads torch.  :class:`AttnWindowState` imports torch when it is built.
"""
from __future__ import annotations

import math
from typing import Any, Dict

KEYS = ("attn_window",)

DEFAULTS: Dict[str, int] = {"attn_window": 0}

MAX_WINDOW = 1 << 30  # the kernels' int32 bounds (q - W, k0 + 256 + W) stay far from overflow


def validate(key: str, value: Any) -> int:
    """The window of ``key`` as an int; ValueError when it is not an integral number in [0, 2^30]."""
    if key not in KEYS:
        raise KeyError(key)
    if isinstance(value, bool):
        raise ValueError(f"{key} must be an integer number of keys, got {value!r}")
    w = float(value)
    if not math.isfinite(w) or w != math.floor(w) or not 0 <= w <= MAX_WINDOW:
        raise ValueError(f"{key} must be an integer in [0, {MAX_WINDOW}] (0: no window), got {value!r}")
    return int(w)


class AttnWindowState:
    """What the windowed attention kernels of one model read on ``device``: ``win``, one int32 (W; 0: no window).
    It is allocated here, never during a capture.  ``set`` is one 4-byte copy through a pinned staging ring (a plain
    copy on the CPU); ``host`` is the copy the torch fallback reads."""

    def __init__(self, device, attn_window: int = 0):
        import torch

        self.device = torch.device(device)
        self.win = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.host: Dict[str, int] = {"attn_window": validate("attn_window", attn_window)}
        self._ring = None
        if self.device.type == "cuda":
            from polyaxon_amd.ops.optim import _PinnedRing

            self._ring = _PinnedRing(width=1)
        self._upload()

    @property
    def W(self) -> int:
        return self.host["attn_window"]

    def _upload(self) -> None:
        import torch

        word = torch.tensor([self.W], dtype=torch.int32)
        if self._ring is None:
            self.win.copy_(word)
        else:  # the ring stages fp32 slots: the word travels as its bit pattern
            self._ring.copy_to(self.win.view(torch.float32), word.view(torch.float32))

    def set(self, **kv) -> None:
        """Validate, merge into the host copy and upload; a rejected call changes nothing."""
        new = {k: validate(k, v) for k, v in kv.items()}
        self.host.update(new)  # only once every value has passed
        self._upload()
