"""Document-masked attention for packed sequences: when several documents share one row of the batch, query ``i``
of row ``b`` sees key ``j`` iff ``start[b][i] <= j <= i`` -- causal attention inside its own document.  The mask is two
int32 ``[B, S]`` device tables shared by all heads, ``start[b][i]`` the first position of ``i``'s document and
``end[b][j]`` one past the last position of ``j``'s, which the document flash-attention kernels
(csrc/attn_kernels.hip ``plx_attn_doc_fwd`` / ``plx_attn_doc_bwd``) read at run time: one captured step follows the
batch from replay to replay, and a query block only visits the key tiles of its documents.

Position ``t`` starts a document iff ``t == 0`` or ``tokens[b][t - 1] == eos_id``: the EOS token belongs to the
document it ends.  Document attention is causal self-attention only (``S == Skv``), so every query keeps its diagonal
key and no row is ever fully masked.  Like the window it is part of the model: it holds in ``eval()`` and in
activation-checkpoint recomputation alike.  Positions are not reset per document.

Validation is pure Python on purpose: polyflow/programs.py calls it, and the scheduler process that imports that
module never loads torch.  :class:`AttnDocState` imports torch when it is built.
"""
from __future__ import annotations

import math
from typing import Any

MAX_TOKEN = (1 << 31) - 1


def validate(value: Any) -> int:
    """The EOS token id as an int; ValueError when it is not an integral number in [0, 2^31)."""
    if isinstance(value, bool):
        raise ValueError(f"attn_doc_eos must be a token id, got {value!r}")
    t = float(value)
    if not math.isfinite(t) or t != math.floor(t) or not 0 <= t <= MAX_TOKEN:
        raise ValueError(f"attn_doc_eos must be an integer token id in [0, {MAX_TOKEN}], got {value!r}")
    return int(t)


class AttnDocState:
    """What the document attention kernels of one model read on ``device``: the ``start`` and ``end`` tables of a
    ``[batch, seq]`` batch, allocated here (never during a capture) and holding "one document per row" until
    ``update`` or ``set_tables`` fills them."""

    def __init__(self, device, batch: int, seq: int, eos_id: int):
        import torch

        self.device = torch.device(device)
        self.eos_id = validate(eos_id)
        self.start = torch.zeros(batch, seq, dtype=torch.int32, device=self.device)
        self.end = torch.full((batch, seq), seq, dtype=torch.int32, device=self.device)
        self._pos = torch.arange(seq, dtype=torch.int32, device=self.device)

    def update(self, tokens) -> None:
        """Fill both tables in place from ``tokens [batch, seq]``.  No host read and no op whose output size depends
        on the data, so it runs inside a captured step: ``start`` is the running maximum of the positions that open
        a document, ``end`` the reversed running minimum of the positions one past an EOS."""
        import torch

        if tuple(tokens.shape) != tuple(self.start.shape):
            raise ValueError(f"tokens {tuple(tokens.shape)} do not match the tables {tuple(self.start.shape)}")
        B, S = self.start.shape
        eos = tokens == self.eos_id
        first = torch.zeros_like(self.start)  # the position itself where it opens a document, else 0
        first[:, 1:] = torch.where(eos[:, :-1], self._pos[1:], 0)
        self.start.copy_(first.cummax(1).values)
        last = torch.where(eos, self._pos + 1, S).flip(1)  # one past the position where it closes one, else S
        self.end.copy_(last.cummin(1).values.flip(1))

    def set_tables(self, start, end) -> None:
        """Copy explicit ``[batch, seq]`` tables in (a packer of the user's own, or a test)."""
        if tuple(start.shape) != tuple(self.start.shape) or tuple(end.shape) != tuple(self.end.shape):
            raise ValueError(f"tables must be {tuple(self.start.shape)}, got {tuple(start.shape)} / {tuple(end.shape)}")
        self.start.copy_(start)
        self.end.copy_(end)
