"""Residual dropout as a device-resident hyper-parameter: the rate is four 32-bit words of device memory, the mask is
never stored -- forward and backward regenerate it from the trainer's device step counter.

Names, defaults and validation are pure Python on purpose: polyflow/programs.py reads the key names from here, and
the scheduler process that imports it never loads torch (tests/test_gpu_free_scheduler.py).  :class:`DropoutState`
imports torch when it is built; :func:`mask_reference` needs numpy only.

The mask contract, shared by the kernels (csrc/rmsnorm.hip ``plx_add_*_drop_*``, ``plx_dropout``) and this host twin:

* device state, 4 x uint32: [0] the threshold ``T = min(round(p * 65536), 65535)``; [1] the bits of the fp32 scale
  ``c = 65536 / (65536 - T)`` (fp64, rounded once: the inverse of the *realised* keep probability, 1.0 exactly at
  T = 0); [2], [3] the Philox key -- a program-level ``dropout_seed`` with the data-parallel rank folded into the
  second word.  The key is not the trial's init seed: snapshots carry no hyper-parameter memory, so a resumed trial
  continues its mask stream from the restored step counter alone, and trials compared with each other see the same
  masks;
* 16-byte vector ``v`` (8 elements; the 64-bit index ``row * d/8 + i``) of site ``site`` at step ``t`` draws
  ``w = Philox4x32-10(counter = (v_lo, v_hi, t, site), key)``; element ``k`` takes the 16-bit half
  ``(w[k >> 1] >> 16 * (k & 1)) & 0xffff`` and is kept iff ``half >= T``;
* sites of an ``n``-layer pre-norm transformer: ``2 l`` after the attention of block ``l``, ``2 l + 1`` after its
  MLP, ``2 n`` the embedding sum;
* forward ``s = bf16(x + (keep ? c * res : 0))``; backward ``dres = bf16(keep ? c * g : +0)`` with ``g`` the fp32
  value ``dx`` is rounded from.  At T = 0 everything is bit for bit the plain add.

Nothing may advance the step counter between a step's forward and its backward: the executor's counter moves in
``plx_record_metric``, the last launch of the step, and the LM trainer's after its optimizer step.
"""
from __future__ import annotations

import math
import struct
from typing import Any, Dict, Tuple

KEYS = ("dropout",)

DEFAULTS: Dict[str, float] = {"dropout": 0.0}


def validate(key: str, value: Any) -> float:
    """The rate of ``key`` as a float; ValueError when it is not a finite number in [0, 1)."""
    if key not in KEYS:
        raise KeyError(key)
    p = float(value)
    if not math.isfinite(p) or not 0.0 <= p < 1.0:
        raise ValueError(f"{key} must be a finite rate in [0, 1), got {value!r}")
    return p


def threshold(p: float) -> int:
    """T of rate ``p``: a 16-bit draw below it is dropped, so the realised rate is T / 65536."""
    return min(int(round(validate("dropout", p) * 65536)), 65535)


def scale(T: int) -> float:
    """The fp32 scale of the kept elements, 65536 / (65536 - T) computed in fp64 and rounded once."""
    if not 0 <= int(T) <= 65535:
        raise ValueError(f"threshold must be in [0, 65535], got {T!r}")
    return struct.unpack("<f", struct.pack("<f", 65536.0 / (65536 - int(T))))[0]


def key_words(seed: int, rank: int = 0) -> Tuple[int, int]:
    """The Philox key of ``dropout_seed`` on data-parallel ``rank``: every rank draws its own masks."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, ((seed >> 32) ^ int(rank)) & 0xFFFFFFFF


def mask_reference(key, step: int, site: int, n_vec: int, T: int):
    """bool [n_vec, 8]: True where element k of 16-byte vector v is kept (the contract in the module docstring)."""
    import numpy as np

    from polyaxon_amd.polytune.sampler import philox4x32_10

    v = np.arange(int(n_vec), dtype=np.uint64)
    w = philox4x32_10((v & np.uint64(0xFFFFFFFF)).astype(np.uint32), (v >> np.uint64(32)).astype(np.uint32),
                      np.full(int(n_vec), int(step) & 0xFFFFFFFF, np.uint32),
                      np.full(int(n_vec), int(site) & 0xFFFFFFFF, np.uint32), int(key[0]), int(key[1]))
    halves = np.stack([(w[k >> 1] >> np.uint32(16 * (k & 1))) & np.uint32(0xFFFF) for k in range(8)], axis=1)
    return halves >= np.uint32(T)


class DropoutState:
    """What the dropout sites of one model read on ``device``:

    ``hp``            4 x int32 (the words of the contract above) that the kernels read at run time, so one captured
                      step serves every rate;
    ``step_counter``  the trainer's device step counter (int32), shared with the optimizer -- not owned here.

    ``hp`` is allocated here, never during a capture.  ``set`` is one 16-byte copy through a pinned staging ring (a
    plain copy on the CPU); ``host`` / ``T`` / ``c`` / ``key`` are the copies the torch fallback reads."""

    def __init__(self, device, step_counter, seed: int = 0, rank: int = 0):
        import torch

        self.device = torch.device(device)
        self.step_counter = step_counter
        self.seed, self.rank = int(seed), int(rank)
        self.hp = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.host: Dict[str, float] = dict(DEFAULTS)
        self._ring = None
        if self.device.type == "cuda":
            from polyaxon_amd.ops.optim import _PinnedRing

            self._ring = _PinnedRing(width=4)
        self._upload()

    @property
    def T(self) -> int:
        return threshold(self.host["dropout"])

    @property
    def c(self) -> float:
        return scale(self.T)

    @property
    def key(self) -> Tuple[int, int]:
        return key_words(self.seed, self.rank)

    def words(self) -> Tuple[int, int, int, int]:
        return (self.T, struct.unpack("<I", struct.pack("<f", self.c))[0]) + self.key

    def _upload(self) -> None:
        import torch

        bits = torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in self.words()], dtype=torch.int32)
        if self._ring is None:
            self.hp.copy_(bits)
        else:  # the ring stages fp32 slots: the words travel as their bit patterns
            self._ring.copy_to(self.hp.view(torch.float32), bits.view(torch.float32))

    def set(self, **kv) -> None:
        """Validate, merge into the host copy and upload; a rejected call changes nothing."""
        new = {k: validate(k, v) for k, v in kv.items()}
        self.host.update(new)  # only once every value has passed
        self._upload()

    def set_rank(self, rank: int) -> None:
        """Fold data-parallel ``rank`` into the key (executor ``enable_dp``)."""
        self.rank = int(rank)
        self._upload()

    def step(self) -> int:
        """The step the next forward draws its masks at; reads the device counter (the torch fallback only)."""
        return int(self.step_counter.reshape(-1)[0].item())
