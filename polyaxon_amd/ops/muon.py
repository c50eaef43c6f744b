"""Muon's orthogonalisation: the batched Newton-Schulz plan (csrc/muon_kernels.hip) and its CPU twin.

For a matrix U (r x c) the update direction is O = NS5(U / (|U|_F + 1e-7)): five iterations of A = X X^T,
B = b A + c A A, X' = a X + B X on X = U (r <= c) or U^T (r > c).  The kernels keep X, A and B as bf16 and accumulate
in fp32; the twin rounds at the same storage points, so the two differ in summation order only.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from polyaxon_amd.ops import _native

COEF = (3.4445, -4.7750, 2.0315)
ITERS = 5


def _bf16(x: torch.Tensor, on: bool) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype) if on else x


def newton_schulz_reference(u: torch.Tensor, dtype: torch.dtype = torch.float64, rounding: bool = True,
                            scale: Optional[float] = None) -> torch.Tensor:
    """The twin of the five iterations on one matrix ``u`` (r x c), computed in ``dtype``.  ``rounding``: round u, A,
    B and every X' to bf16 as the kernels store them (u unscaled: 1 / (|u| + 1e-7) enters as the first iteration's
    epilogue scalars, its square on A and itself on X').  ``scale``: that factor, when the caller already has it."""
    a, b, c = COEF
    u = _bf16(u.to(dtype), rounding)
    s = 1.0 / (u.norm() + 1e-7) if scale is None else torch.tensor(scale, dtype=dtype)
    tall = u.shape[0] > u.shape[1]
    x = u.T if tall else u
    for it in range(ITERS):
        f = s if it == 0 else 1.0
        A = _bf16((x @ x.T) * (f * f), rounding)
        B = _bf16(c * (A @ A) + b * A, rounding)
        x = _bf16((B @ x + a * x) * f, rounding)
    return x.T if tall else x


class MuonPlan:
    """Everything the Muon launches need for a fixed set of matrices, built once: the bf16 workspace (per matrix two
    X buffers, A and B), the per-matrix descriptors, the tile tables of the three stages (stages 1 and 2: upper
    triangle only) and the chunk table of the momentum / update passes.  ``shapes[p]`` = (rows, cols) of matrix p,
    ``offsets[p]`` its first element in the flat buffers.  Nothing is allocated after construction."""

    def __init__(self, shapes: Sequence[Tuple[int, int]], offsets: Sequence[int], device):
        lib = _native.lib("plx_muon")
        _native.check(lib.plx_muon_prepare(), "plx_muon_prepare")
        assert lib.plx_muon_problem_size() == 64
        tile, chunk = lib.plx_muon_tile(), lib.plx_muon_chunk()
        self.shapes, self.offsets = [tuple(s) for s in shapes], list(offsets)
        desc, sym, full, rect = [], [], [], []
        lo, hi, owner, first, count = [], [], [], [], []
        off = 0
        self._where: List[Tuple[int, int, int, int]] = []
        for p, ((r, c), flat) in enumerate(zip(self.shapes, self.offsets)):
            m = min(r, c)
            x0, x1, a, b = off, off + r * c, off + 2 * r * c, off + 2 * r * c + m * m
            off = b + m * m
            self._where.append((x0, x1, a, b))
            desc.append([x0, x1, a, b, r, c, flat, 0])
            tm = -(-m // tile)
            full += [[p, i, j, 0] for i in range(tm) for j in range(tm)]
            sym += [[p, i, j, 0] for i in range(tm) for j in range(i, tm)]
            rect += [[p, i, j, 0] for i in range(-(-r // tile)) for j in range(-(-c // tile))]
            first.append(len(lo))
            for s in range(flat, flat + r * c, chunk):
                lo.append(s)
                hi.append(min(s + chunk, flat + r * c))
                owner.append(p)
            count.append(len(lo) - first[-1])

        def dev(rows, dtype):
            return torch.tensor(rows, dtype=dtype, device=device)

        self.n_problems, self.n_chunks = len(desc), len(lo)
        self.problems = dev(desc, torch.int64)
        self.tiles_sym, self.tiles_full, self.tiles_rect = (dev(t, torch.int32) for t in (sym, full, rect))
        self.chunk_lo, self.chunk_hi = dev(lo, torch.int64), dev(hi, torch.int64)
        self.chunk_problem = dev(owner, torch.int32)
        self.first, self.count = dev(first, torch.int32), dev(count, torch.int32)
        self.ws = torch.zeros(off, dtype=torch.bfloat16, device=device)
        self.partials = torch.zeros(max(self.n_chunks, 1), dtype=torch.float32, device=device)
        self.scale = torch.ones(max(self.n_problems, 1), dtype=torch.float32, device=device)

    def x(self, p: int, buf: int = 0) -> torch.Tensor:
        r, c = self.shapes[p]
        return self.ws[self._where[p][buf]:][: r * c].view(r, c)

    def a(self, p: int) -> torch.Tensor:
        m = min(self.shapes[p])
        return self.ws[self._where[p][2]:][: m * m].view(m, m)

    def b(self, p: int) -> torch.Tensor:
        m = min(self.shapes[p])
        return self.ws[self._where[p][3]:][: m * m].view(m, m)

    def stage(self, stage: int, first: bool, xin: int, stream: int, triangle: bool = True) -> None:
        """One stage over every matrix.  ``triangle=False`` (stages 1, 2): every tile is computed, none mirrored."""
        tiles = self.tiles_rect if stage == 3 else (self.tiles_sym if triangle else self.tiles_full)
        _native.check(_native.lib("plx_muon").plx_muon_stage(
            stage, int(first), self.problems.data_ptr(), tiles.data_ptr(), tiles.shape[0], self.ws.data_ptr(),
            self.scale.data_ptr(), xin, int(triangle), stream), "plx_muon_stage")

    def iterate(self, stream: int) -> int:
        """The 15 stage launches: X buffer 0 (u) and ``scale`` in, O in the X buffer whose index is returned."""
        for it in range(ITERS):
            for stage in (1, 2, 3):
                self.stage(stage, it == 0, it & 1, stream)
        return ITERS & 1

    def step(self, flat, mom: torch.Tensor, hp: torch.Tensor, sched: Optional[torch.Tensor],
             state: Optional[torch.Tensor], stream: int) -> None:
        """Momentum, norms, the iteration and the weight update of every matrix, queued on ``stream``."""
        lib = _native.lib("plx_muon")
        lp = flat.lp_params is not None
        g = flat.lp_grads if lp else flat.grads
        st = state.data_ptr() if state is not None else None
        tables = (self.chunk_lo.data_ptr(), self.chunk_hi.data_ptr(), self.chunk_problem.data_ptr(), self.n_chunks,
                  self.problems.data_ptr(), self.ws.data_ptr())
        _native.check(lib.plx_muon_momentum(int(lp), g.data_ptr(), mom.data_ptr(), *tables, hp.data_ptr(), st,
                                            self.partials.data_ptr(), stream), "plx_muon_momentum")
        _native.check(lib.plx_muon_norms(self.partials.data_ptr(), self.first.data_ptr(), self.count.data_ptr(),
                                         self.n_problems, self.scale.data_ptr(), stream), "plx_muon_norms")
        out = self.iterate(stream)
        _native.check(lib.plx_muon_update(flat.params.data_ptr(), flat.lp_params.data_ptr() if lp else None, *tables,
                                          out, hp.data_ptr(), sched.data_ptr() if sched is not None else None, st,
                                          stream), "plx_muon_update")
