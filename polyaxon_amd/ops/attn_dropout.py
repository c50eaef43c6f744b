"""Attention dropout (GPT-2's ``attn_pdrop``) as a device-resident hyper-parameter: dropout on the softmax
probabilities inside flash attention.  The rate is four 32-bit words of device memory, the mask is never stored --
the forward and the three backward passes of csrc/attn_kernels.hip regenerate it from the trainer's device step
counter, so one captured step serves every rate.

Names, defaults and validation are pure Python on purpose: polyflow/programs.py reads the key names from here, and
the scheduler process that imports it never loads torch (tests/test_gpu_free_scheduler.py).  :class:`AttnDropoutState`
imports torch when it is built; :func:`mask_reference` needs numpy only.

The mask contract, shared by the kernels (``plx_attn_drop_fwd`` / ``plx_attn_drop_bwd``) and this host twin:

* device state, 4 x uint32: [0] the threshold ``T = min(round(p * 256), 255)``; [1] the bits of the fp32 scale
  ``c = 256 / (256 - T)`` (fp64, rounded once: the inverse of the *realised* keep probability ``1 - T / 256``, 1.0
  exactly at T = 0); [2], [3] the Philox key, ``dropout.key_words(dropout_seed, rank)``.  The resolution is 8 bits so
  that one Philox call covers a square 4 x 4 block of the score matrix;
* element ``(b, h, q, k)`` (``h`` the query head, ``q`` / ``k`` absolute query / key indices) of layer ``l`` at step
  ``t`` draws ``w = Philox4x32-10(counter = (q >> 2, k >> 2, t, 0x80000000 | (l << 16) | (b * H + h)), key)``, takes
  the byte ``(w[q & 3] >> 8 * (k & 3)) & 0xff`` and is kept iff ``byte >= T``.  Bit 31 of the fourth counter word
  keeps these streams apart from the residual sites of ops/dropout.py (``site <= 2 n``).  The block is the same
  whichever way a kernel holds the scores (a lane owning a query and 4 keys, or a key and 4 queries) and does not
  depend on any tile size;
* valid for ``b * H + h < 65536`` and ``l < 32768``;
* math, with ``M`` the mask and ``P`` the softmax probabilities: the softmax statistics (row max, row sum, the stored
  ``lse2``) use the undropped ``P``; ``O = (c M o P) V``; backward ``dP = c M o (dO V^T)``, ``dS = P o (dP - delta)``
  with ``delta = rowsum(dO o O)`` unchanged, ``dV = (c M o P)^T dO``.  At T = 0 everything is bit for bit the plain
  attention.

Nothing may advance the step counter between a step's forward and its backward (the rule of ops/dropout.py).
"""
from __future__ import annotations

import math
import struct
from typing import Any, Dict, Tuple

from polyaxon_amd.ops.dropout import key_words

KEYS = ("attn_dropout",)

DEFAULTS: Dict[str, float] = {"attn_dropout": 0.0}

STREAM_BIT = 0x80000000  # bit 31 of the fourth counter word: attention streams, apart from the residual sites
MAX_BH = 65536           # b * H + h below this
MAX_LAYERS = 32768       # l below this


def validate(key: str, value: Any) -> float:
    """The rate of ``key`` as a float; ValueError when it is not a finite number in [0, 1)."""
    if key not in KEYS:
        raise KeyError(key)
    p = float(value)
    if not math.isfinite(p) or not 0.0 <= p < 1.0:
        raise ValueError(f"{key} must be a finite rate in [0, 1), got {value!r}")
    return p


def threshold(p: float) -> int:
    """T of rate ``p``: an 8-bit draw below it is dropped, so the realised rate is T / 256."""
    return min(int(round(validate("attn_dropout", p) * 256)), 255)


def scale(T: int) -> float:
    """The fp32 scale of the kept probabilities, 256 / (256 - T) computed in fp64 and rounded once."""
    if not 0 <= int(T) <= 255:
        raise ValueError(f"threshold must be in [0, 255], got {T!r}")
    return struct.unpack("<f", struct.pack("<f", 256.0 / (256 - int(T))))[0]


def stream_word(layer: int, bh: int) -> int:
    """The fourth counter word of layer ``layer``, flattened batch x query head ``bh``."""
    if not 0 <= int(layer) < MAX_LAYERS or not 0 <= int(bh) < MAX_BH:
        raise ValueError(f"attention dropout needs layer < {MAX_LAYERS} and b * H + h < {MAX_BH}, got {layer}, {bh}")
    return STREAM_BIT | (int(layer) << 16) | int(bh)


def mask_reference(key, step: int, layer: int, bh: int, S: int, Skv: int, T: int, q0: int = 0, k0: int = 0):
    """bool [S, Skv]: True where the probability of query ``q0 + i``, key ``k0 + j`` is kept (the contract in the
    module docstring)."""
    import numpy as np

    from polyaxon_amd.polytune.sampler import philox4x32_10

    q = np.arange(int(q0), int(q0) + int(S), dtype=np.int64)
    k = np.arange(int(k0), int(k0) + int(Skv), dtype=np.int64)
    qb, kb = np.unique(q >> 2), np.unique(k >> 2)
    c0 = np.repeat(qb, len(kb)).astype(np.uint32)
    c1 = np.tile(kb, len(qb)).astype(np.uint32)
    n = c0.size
    w = philox4x32_10(c0, c1, np.full(n, int(step) & 0xFFFFFFFF, np.uint32),
                      np.full(n, stream_word(layer, bh), np.uint32), int(key[0]), int(key[1]))
    w = np.stack([np.asarray(x, np.uint32) for x in w], 0).reshape(4, len(qb), len(kb))
    qi, ki = (q >> 2) - qb[0], (k >> 2) - kb[0]
    word = w[(q & 3)[:, None], qi[:, None], ki[None, :]]
    byte = (word >> (8 * (k & 3)).astype(np.uint32)[None, :]) & np.uint32(0xFF)
    return byte >= np.uint32(T)


class AttnDropoutState:
    """What the attention kernels of one model read on ``device``:

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
        return threshold(self.host["attn_dropout"])

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
