"""Fused flat-buffer optimizers with device-resident hyper-parameters.

The hyper-parameters (lr, momentum, weight decay, ...) live in a small fp32 device tensor that the kernel
reads at run time.  A trial executor therefore changes a trial's hyper-parameters with one 32-byte H2D
copy and keeps replaying the SAME captured hipGraph — the graph never has to be re-captured per trial,
which is what makes a warm per-GPU trial executor cheap (SURVEY.md §7.1 polyflow; BASELINE.md "reference
design constants": every reference trial pays pod start + 1 s task hops instead).

Global-norm gradient clipping (``max_grad_norm=``, opt-in) follows the same rule: the threshold is one more slot of
that tensor, and the norm, the scale and the skip of a non-finite step are computed and consumed on the device
(``plx_gradnorm_partials`` / ``plx_gradnorm_finalize`` / the ``*_clip`` optimizer kernels), so a captured step
clips every trial to its own threshold without a host sync or a re-capture.

Learning-rate schedules (``lr_schedule=``, opt-in) are device data too: an 8-float ``sched`` tensor (base LR, kind,
warm-up, horizon, floor, decay) that ``plx_lr_schedule`` turns into ``hp[0]`` from the device step counter, one tiny
launch ahead of the step's optimizer launches.  A trial changes its schedule -- kind included -- with one more
32-byte copy; snapshots restore the step counter, so a resumed trial continues its curve with nothing else saved.

Layer-wise trust ratios (``FusedSGD(trust_coef=)``: LARS; ``FusedAdamW(lamb=True)``: LAMB; opt-in) keep to it as
well: the per-tensor norms, the ratios and the update are three launches over a chunk table built once
(csrc/layerwise_kernels.hip), in a fixed summation order, and ``trust_coef`` is one more slot of the tensor.

Muon (``FusedAdamW(muon=<parameter names>)``, opt-in) moves the named weight matrices from AdamW to momentum plus a
Newton-Schulz orthogonalised update: one batched launch per stage over every such matrix (csrc/muon_kernels.hip,
ops/muon.py), with ``muon_lr`` and ``muon_momentum`` as two more slots of the tensor.

On CPU (no native library) the same update is computed with torch ops; tests compare the two.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from polyaxon_amd.ops import _native, lr_schedule as _lrs, muon as _muon, side_stream
from polyaxon_amd.ops.flat import FlatParams


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class _PinnedRing:
    """Preallocated pinned staging slots for the per-trial hyper-parameter H2D copies.  ``tensor.pin_memory()``
    per call went through the caching host allocator, which allocates fresh pinned memory (a synchronising
    hipHostMalloc) while earlier copies are still queued -- with the host running trials ahead of the GPU that
    stalled it, and the GPU then idled at every trial start waiting for the host's next launches.  A slot is
    reused only after the event recorded behind its copy has completed (it nearly always has: 64 trials later)."""

    def __init__(self, slots: int = 64, width: int = 8):
        self.buf = torch.zeros(slots, width, dtype=torch.float32).pin_memory()
        self.events = [None] * slots
        self.i = 0

    def copy_to(self, dst: torch.Tensor, values) -> None:
        i = self.i
        self.i = (i + 1) % len(self.events)
        ev = self.events[i]
        if ev is not None:
            ev.synchronize()
        # an fp32 tensor is staged as it is: raw 32-bit words viewed as fp32 keep their bits (ops/dropout.py)
        self.buf[i, : len(values)] = values if torch.is_tensor(values) else torch.tensor(values, dtype=torch.float32)
        dst.copy_(self.buf[i, : dst.numel()], non_blocking=True)
        ev = self.events[i] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dst.device))
        self.events[i] = ev


def _set_hp(opt, values, dst: Optional[torch.Tensor] = None) -> None:
    """``dst`` (default ``opt.hp``; the 8-float ``sched`` tensor of a scheduled optimizer) := ``values``."""
    dst = opt.hp if dst is None else dst
    if not dst.is_cuda:
        dst.copy_(torch.tensor(values, dtype=torch.float32))
        return
    ring = getattr(opt, "_ring", None)
    if ring is None:
        ring = opt._ring = _PinnedRing(width=opt.hp.numel())
    ring.copy_to(dst, values)


class _GradClip:
    """Global-norm gradient clipping with a device-resident threshold (hp slot 5, ``max_grad_norm``).

    Before the update, one ``plx_gradnorm_partials`` launch per gradient buffer (lp mode: the bf16 decay segment and
    the fp32 tail, into disjoint slot ranges) writes per-workgroup sums of squares in a fixed order, and
    ``plx_gradnorm_finalize`` turns them and the threshold into the 4-float device ``state``: [0] the step's total
    norm before clipping, [1] the scale the ``*_clip`` optimizer kernels apply, [2] steps skipped since the last
    reset, [3] 1.0 when this step is skipped (non-finite norm: the kernels then only zero the gradients).
    scale = min(1, max_norm / (norm + 1e-6)), ``torch.nn.utils.clip_grad_norm_``'s; max_norm <= 0 measures the norm
    and scales by exactly 1.0.  No host sync, no atomics; every buffer is allocated here, never during a capture."""

    SLOT = 5

    def __init__(self, flat: FlatParams):
        self.flat = flat
        dev = flat.device
        self.state = torch.zeros(4, dtype=torch.float32, device=dev)
        bufs = [flat.grads] if flat.lp_grads is None else [flat.lp_grads, flat.grads]
        self.ranges = []  # (gradient buffer, is_bf16, first partial slot, slots)
        n_slots = 0
        if flat.params.is_cuda:
            for b in bufs:
                if b.numel():
                    k = _native.size("plx_train", "plx_gradnorm_blocks", b.numel())
                    self.ranges.append((b, int(b.dtype == torch.bfloat16), n_slots, k))
                    n_slots += k
        self.n_slots = n_slots
        self.partials = torch.zeros(max(n_slots, 1), dtype=torch.float32, device=dev)

    def measure(self, hp: torch.Tensor, stream: int) -> None:
        """Queue the norm pass and the finalize on ``stream`` (GPU)."""
        lib = _native.lib("plx_train")
        # the pass reads every gradient slot: after the side-stream weight-gradient writers (ops/side_stream.py)
        side_stream.join(self.flat.device)
        for buf, is_bf16, first, _ in self.ranges:
            _native.check(lib.plx_gradnorm_partials(buf.data_ptr(), is_bf16, buf.numel(),
                                                    self.partials.data_ptr() + 4 * first, stream),
                          "plx_gradnorm_partials")
        _native.check(lib.plx_gradnorm_finalize(self.partials.data_ptr(), self.n_slots, hp.data_ptr(),
                                                self.state.data_ptr(), stream), "plx_gradnorm_finalize")

    @torch.no_grad()
    def measure_reference(self, hp: torch.Tensor) -> Optional[float]:
        """The same state update in torch ops (CPU).  Returns the scale, or None when the step is skipped."""
        f = self.flat
        g = f.grads if f.lp_grads is None else torch.cat([f.lp_grads.float(), f.grads])
        norm = g.double().norm().float()
        max_norm = hp[self.SLOT]
        self.state[0] = norm
        if not bool(torch.isfinite(norm)):
            self.state[1] = 0.0
            self.state[2] += 1.0
            self.state[3] = 1.0
            return None
        scale = torch.ones((), dtype=torch.float32)
        if float(max_norm) > 0.0:
            scale = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        self.state[1] = scale
        self.state[3] = 0.0
        return float(scale)

    def stats(self) -> Dict[str, float]:
        st = self.state.tolist()  # device -> host: synchronises
        return {"grad_norm": st[0], "scale": st[1], "skipped": st[2]}

    def reset(self) -> None:
        self.state.zero_()


class _Clipping:
    """The ``max_grad_norm`` surface the fused optimizers share.  ``max_grad_norm=None`` (default): no clipping --
    the hyper-parameter does not exist, no buffer is allocated, the launches are the ones without it."""

    _clip: Optional[_GradClip] = None

    def _init_clip(self, flat: FlatParams, max_grad_norm: Optional[float]) -> None:
        if max_grad_norm is None:
            return
        assert len(type(self).HP) == _GradClip.SLOT
        self.HP = type(self).HP + ("max_grad_norm",)  # this instance only: hp slot 5
        self._clip = _GradClip(flat)

    @property
    def clipping(self) -> bool:
        return self._clip is not None

    def _need_clip(self) -> _GradClip:
        if self._clip is None:
            raise RuntimeError("gradient clipping is off: build the optimizer with max_grad_norm=<number>")
        return self._clip

    def grad_norm(self) -> torch.Tensor:
        """The last step's global gradient norm, before clipping: a 0-dim view of the device state (no sync)."""
        return self._need_clip().state[0]

    def clip_stats(self) -> Dict[str, float]:
        """Host floats {grad_norm, scale, skipped (steps since the last reset)} of the last step; synchronises."""
        return self._need_clip().stats()


class _LayerNorms:
    """The device side of the layer-wise trust ratios (``FusedSGD(trust_coef=)``: LARS; ``FusedAdamW(lamb=True)``:
    LAMB; csrc/layerwise_kernels.hip).  The decay segments -- every tensor of rank 2 or higher -- are cut into chunks
    of ``plx_lw_chunk()`` elements that never cross a segment: per chunk [lo, hi) and its segment, per segment its
    first chunk and chunk count.  A step is three launches over that table: two sums of squares per chunk
    (``plx_lw_norms``; LAMB's also advances and stores the moments), one ratio per segment (``plx_lw_ratios``), the
    update of every chunk with its segment's ratio (``plx_lw_update``).  The padding after a segment's ``numel`` is
    in no chunk: it is in no norm and is never written.  The 1-D tail keeps the plain update.  No host sync, no
    atomics, a fixed summation order; every buffer is allocated here, never during a capture."""

    LARS, LAMB, LAMB_LP = 0, 1, 2

    def __init__(self, flat: FlatParams, mode: int):
        self.flat = flat
        self.mode = mode
        self.segs = [s for s in flat.segments if s.decay]
        if not flat.params.is_cuda:
            return
        chunk = _native.lib("plx_layerwise").plx_lw_chunk()
        lo, hi, seg, first, count = [], [], [], [], []
        for i, s in enumerate(self.segs):
            end = s.offset + s.numel
            first.append(len(lo))
            for c in range(s.offset, end, chunk):
                lo.append(c)
                hi.append(min(c + chunk, end))
                seg.append(i)
            count.append(len(lo) - first[-1])
        dev = flat.device
        self.n_chunks, self.n_segs = len(lo), len(self.segs)
        self.chunk_lo = torch.tensor(lo, dtype=torch.int64, device=dev)
        self.chunk_hi = torch.tensor(hi, dtype=torch.int64, device=dev)
        self.chunk_seg = torch.tensor(seg, dtype=torch.int32, device=dev)
        self.seg_first = torch.tensor(first, dtype=torch.int32, device=dev)
        self.seg_count = torch.tensor(count, dtype=torch.int32, device=dev)
        self.partials = torch.zeros(2 * max(self.n_chunks, 1), dtype=torch.float32, device=dev)
        self.ratio = torch.ones(max(self.n_segs, 1), dtype=torch.float32, device=dev)

    def step(self, m: torch.Tensor, v: Optional[torch.Tensor], hp: torch.Tensor, step: torch.Tensor,
             clip: Optional[_GradClip], stream: int) -> None:
        """Queue the three passes over the decay segments on ``stream`` (GPU).  ``m``: the momentum buffer (LARS) or
        ``exp_avg``; ``v``: ``exp_avg_sq`` (LAMB).  ``clip``: its state must already be this step's."""
        f, lib = self.flat, _native.lib("plx_layerwise")
        side_stream.join(f.device)  # the norm pass reads every gradient slot (as _GradClip.measure)
        lp = self.mode == self.LAMB_LP
        g = (f.lp_grads if lp else f.grads).data_ptr()
        vp = v.data_ptr() if v is not None else None
        state = clip.state.data_ptr() if clip is not None else None
        _native.check(lib.plx_lw_norms(self.mode, f.params.data_ptr(), g, m.data_ptr(), vp, self.chunk_lo.data_ptr(),
                                       self.chunk_hi.data_ptr(), self.n_chunks, hp.data_ptr(), step.data_ptr(), state,
                                       self.partials.data_ptr(), stream), "plx_lw_norms")
        _native.check(lib.plx_lw_ratios(int(self.mode != self.LARS), self.partials.data_ptr(),
                                        self.seg_first.data_ptr(), self.seg_count.data_ptr(), self.n_segs,
                                        hp.data_ptr(), state, self.ratio.data_ptr(), stream), "plx_lw_ratios")
        _native.check(lib.plx_lw_update(self.mode, f.params.data_ptr(), g, m.data_ptr(), vp,
                                        f.lp_params.data_ptr() if lp else None, self.chunk_lo.data_ptr(),
                                        self.chunk_hi.data_ptr(), self.chunk_seg.data_ptr(), self.n_chunks,
                                        self.ratio.data_ptr(), hp.data_ptr(), step.data_ptr(), state, stream),
                      "plx_lw_update")

    def spans(self):
        """(lo, hi) of every decay segment's real elements (the CPU twins)."""
        return [(s.offset, s.offset + s.numel) for s in self.segs]


class _Layerwise:
    """The layer-wise surface the fused optimizers share.  Off (default): nothing exists -- no table, no buffer, the
    launches are the ones without it.  On, a bucket can cut a segment, so the per-bucket updates
    (``step_range_``, ``FlatDDP(optimizer=...)``, ZeRO-1) cannot see a whole norm and are refused."""

    _lw: Optional[_LayerNorms] = None
    _mu = None  # FusedAdamW(muon=): the Muon segments and their plan
    _in_backward = False

    def _init_layerwise(self, flat: FlatParams, mode: Optional[int], key: Optional[str] = None) -> None:
        if mode is None:
            return
        if key is not None:  # a hyper-parameter of its own, in the hp slot after max_grad_norm's
            if len(self.HP) == _GradClip.SLOT:
                self.HP = self.HP + ("_slot5",)  # no clipping: slot 5 stays 0 and `key` still lands in slot 6
            self.HP = self.HP + (key,)  # this instance only
        self._lw = _LayerNorms(flat, mode)

    @property
    def layerwise(self) -> bool:
        return self._lw is not None

    def _no_ranges(self, what: str) -> None:
        if self._lw is not None:
            raise ValueError(f"a layer-wise optimizer (LARS / LAMB) needs every segment's whole norm before any "
                             f"update: it has no {what} (step_range_, FlatDDP(optimizer=...), ZeRO-1)")
        if self._mu is not None:
            raise ValueError(f"Muon orthogonalises every selected matrix's whole update: it has no {what} "
                             f"(step_range_, FlatDDP(optimizer=...), ZeRO-1)")

    # set by FlatDDP(optimizer=...): the update runs per gradient bucket during the backward (step_range_), and
    # step_() only closes the step's bookkeeping
    @property
    def in_backward(self) -> bool:
        return self._in_backward

    @in_backward.setter
    def in_backward(self, on: bool) -> None:
        if on:
            self._no_ranges("per-bucket update inside the backward")
        self._in_backward = bool(on)


class _MuonSegments:
    """The host side of ``FusedAdamW(muon=)``: the named segments (rank-2 decay segments, both dimensions multiples of
    8, so every vector access of the kernels is whole), the contiguous runs of every other flat element, which keep
    AdamW (in lp mode cut at the bf16 / fp32 boundary), and on the GPU the plan of ops/muon.py."""

    LR, MOMENTUM = 6, 7  # hp slots

    def __init__(self, flat: FlatParams, names):
        by_name = {s.name: s for s in flat.segments}
        self.segs = []
        for name in names:
            seg = by_name.get(name)
            if seg is None:
                raise ValueError(f"muon: no parameter named {name!r}")
            if not seg.decay or len(seg.shape) != 2 or seg.shape[0] % 8 or seg.shape[1] % 8:
                raise ValueError(f"muon: {name!r} {tuple(seg.shape)} is no weight matrix with both dimensions "
                                 f"multiples of 8")
            self.segs.append(seg)
        self.segs.sort(key=lambda s: s.offset)
        cuts = [flat.n_decay] if flat.lp_params is not None else []
        self.runs, at = [], 0
        for lo, hi in [(s.offset, s.offset + s.numel) for s in self.segs] + [(flat.numel, flat.numel)]:
            for edge in cuts + [lo]:
                if at < edge <= lo:
                    self.runs.append((at, edge))
                    at = edge
            at = hi
        self.plan = None
        if flat.params.is_cuda:
            self.plan = _muon.MuonPlan([s.shape for s in self.segs], [s.offset for s in self.segs], flat.device)

    def spans(self):
        return [(s.offset, s.offset + s.numel, s.shape) for s in self.segs]


def lr_factor(kind, s, W, T, m, gamma, E) -> torch.Tensor:
    """The factor ``plx_lr_schedule`` multiplies the base LR by at ``s`` completed steps, in torch float32 (the CPU
    path, and the twin the tests hold the kernel against).  ``kind``: a name or code of ops/lr_schedule.py KINDS;
    W warm-up steps, T horizon (``lr_total_steps``), m ``min_lr_ratio``, gamma / E the ``step`` kind's decay.

    ``s < W``: (s + 1) / W.  After it, with p = clamp((s - W) / max(1, T - W), 0, 1): constant 1; linear
    1 - (1 - m) p; cosine m + (1 - m) (1 + cos(pi p)) / 2; step max(m, gamma^((s - W) // max(1, E))); inv_sqrt
    max(m, sqrt(max(W, 1) / (s + 1))).  Linear and cosine hold 1 when T <= W (no horizon) and are exactly m from
    s = T on.  Wherever the factor is 1 it is exactly 1.0, so ``base_lr * factor`` is then bitwise ``base_lr``."""
    def f32(x):
        return torch.tensor(float(x), dtype=torch.float32)

    code = _lrs.kind_code(kind)
    s, W, E = int(s), int(W), int(E)
    one, sf, Wf, Tf, m, gamma = f32(1.0), f32(s), f32(W), f32(T), f32(m), f32(gamma)
    if s < W:
        return one if s + 1 == W else (sf + 1.0) / Wf
    if code in (1, 2):
        if float(Tf) <= W or float(m) == 1.0:
            return one
        p = (sf - Wf) / (Tf - Wf)
        if float(p) <= 0.0:
            return one
        if float(p) >= 1.0:
            return m
        if code == 1:
            return 1.0 - (1.0 - m) * p
        return m + (1.0 - m) * 0.5 * (1.0 + torch.cos(f32(math.pi) * p))
    if code == 3:
        k = (s - W) // max(1, E)
        return one if k == 0 else torch.maximum(m, torch.pow(gamma, f32(k)))
    if code == 4:
        w = f32(max(W, 1))
        return one if s + 1 == max(W, 1) else torch.maximum(m, torch.sqrt(w / (sf + 1.0)))
    return one


class _LrSchedule:
    """The device side of ``lr_schedule=``: the 8-float ``sched`` tensor -- [0] base LR, [1] kind code, [2]
    ``warmup_steps``, [3] ``lr_total_steps``, [4] ``min_lr_ratio``, [5] ``lr_decay_gamma``, [6] ``lr_decay_every``,
    [7] 0 -- and the launch that evaluates it into ``hp[0]``.  Allocated here, never during a capture."""

    def __init__(self, flat: FlatParams):
        self.sched = torch.zeros(8, dtype=torch.float32, device=flat.device)
        self.queued = False  # per-bucket updates: this step's evaluation is already on the optimizer stream

    def values(self, host: Dict[str, float]):
        return [host["lr"]] + [host[k] for k in _lrs.KEYS] + [0.0]

    def evaluate(self, hp: torch.Tensor, step: torch.Tensor, stream: Optional[int]) -> None:
        """hp[0] = base LR x factor(step): one ``plx_lr_schedule`` launch on ``stream`` (GPU), torch float32 on CPU."""
        if not hp.is_cuda:
            v = self.sched.tolist()
            hp[0] = self.sched[0] * lr_factor(int(v[1]), int(step.item()), *v[2:7])
            return
        st = stream if stream is not None else _stream_ptr(hp)
        _native.check(_native.lib("plx_train").plx_lr_schedule(self.sched.data_ptr(), step.data_ptr(), hp.data_ptr(),
                                                               st), "plx_lr_schedule")


class _Scheduled:
    """The ``lr_schedule`` surface the fused optimizers share.  ``lr_schedule=None`` (default): no schedule -- the
    hyper-parameters do not exist, nothing is allocated, the launches are the ones without it.  With a kind name
    this instance's ``HP`` gains ops/lr_schedule.py KEYS, ``lr`` becomes the base LR, and every step evaluates the
    schedule on the device before its update; ``set_hparams(lr_schedule=<name or code>, ...)`` changes all of it,
    the kind included, per trial."""

    _sched: Optional[_LrSchedule] = None

    def _init_sched(self, flat: FlatParams, lr_schedule: Optional[str]) -> Dict[str, float]:
        """Returns the schedule hyper-parameters the constructor's first ``set_hparams`` sets (none when off)."""
        if lr_schedule is None:
            return {}
        code = _lrs.kind_code(lr_schedule)
        self.HP = self.HP + _lrs.KEYS  # this instance only; they live in ``sched``, not in ``hp``
        self._sched = _LrSchedule(flat)
        return dict(_lrs.DEFAULTS, lr_schedule=code)

    @property
    def scheduled(self) -> bool:
        return self._sched is not None

    def _set_hparams(self, what: str, hp) -> None:
        """Validate, merge into the host copy and upload: ``hp`` (every key that is no schedule key, in ``HP``
        order) and, for a scheduled optimizer, ``sched`` -- both through the pinned ring."""
        vals = getattr(self, "_hp_host", None) or {k: 0.0 for k in self.HP}
        new = {}
        for k, v in hp.items():
            if k not in self.HP:
                raise KeyError(f"unknown {what} hyper-parameter {k!r}")
            new[k] = _lrs.validate(k, v) if k in _lrs.KEYS else float(v)
        vals.update(new)  # only once every value has passed
        self._hp_host = vals
        keys = [k for k in self.HP if k not in _lrs.KEYS] if self._sched is not None else self.HP
        _set_hp(self, [vals[k] for k in keys] + [0.0] * (8 - len(keys)))
        if self._sched is not None:
            _set_hp(self, self._sched.values(vals), self._sched.sched)

    def _schedule_lr(self, stream: Optional[int] = None) -> None:
        if self._sched is not None:
            self._sched.evaluate(self.hp, self.step, stream)

    def current_lr(self) -> torch.Tensor:
        """The learning rate of the last step (scheduled: base LR x factor at that step; before the first step, and
        without a schedule, ``lr`` itself): the 0-dim view ``hp[0]`` of the device hyper-parameters (no sync)."""
        return self.hp[0]


class FusedSGD(_Clipping, _Layerwise, _Scheduled):
    """SGD with momentum / nesterov / dampening and weight decay on the decay segment only; with ``trust_coef`` LARS:
    per decay segment r = trust_coef |w| / (|g| + wd |w| + 1e-8) (1 unless both norms are positive) scales
    d = r (g + wd w) ahead of the momentum rule."""

    HP = ("lr", "momentum", "weight_decay", "nesterov", "dampening")

    def __init__(self, flat: FlatParams, lr: float = 0.1, momentum: float = 0.9, weight_decay: float = 1e-4,
                 nesterov: bool = False, dampening: float = 0.0, step_counter: Optional[torch.Tensor] = None,
                 max_grad_norm: Optional[float] = None, lr_schedule: Optional[str] = None,
                 trust_coef: Optional[float] = None):
        """``max_grad_norm``: a number enables global-norm gradient clipping for the optimizer's lifetime (a device
        hyper-parameter like the others; 0 = measure the norm, no limit); None: no clipping at all.
        ``lr_schedule``: a kind name (ops/lr_schedule.py KINDS) enables the device-resident LR schedule for the
        optimizer's lifetime, ``lr`` being its base LR; None: constant ``lr``, no schedule at all.
        ``trust_coef``: a number enables LARS on the decay segments for the optimizer's lifetime (a device
        hyper-parameter like the others, hp slot 6); None: plain SGD, nothing of it exists."""
        self.flat = flat
        dev = flat.device
        self.momentum_buf = torch.zeros_like(flat.params)
        self.hp = torch.zeros(8, dtype=torch.float32, device=dev)
        # step counter shared with the metric ring: 0 right after reset() => momentum := grad
        self.step = step_counter if step_counter is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        self._init_clip(flat, max_grad_norm)
        self._init_layerwise(flat, None if trust_coef is None else _LayerNorms.LARS, "trust_coef")
        sched = self._init_sched(flat, lr_schedule)
        self.set_hparams(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                         dampening=dampening, **({"max_grad_norm": max_grad_norm} if self.clipping else {}),
                         **({"trust_coef": trust_coef} if self.layerwise else {}), **sched)

    def set_hparams(self, **hp) -> None:
        self._set_hparams("SGD", hp)

    def reset_state(self) -> None:
        if self.flat.params.is_cuda:
            _native.check(_native.lib("plx_train").plx_zero_flat(
                self.momentum_buf.data_ptr(), self.momentum_buf.numel(), _stream_ptr(self.hp)), "plx_zero_flat")
        else:
            self.momentum_buf.zero_()
        if self._clip is not None:
            self._clip.reset()

    def step_(self) -> None:
        f = self.flat
        f.grads_consumed()
        if f.lp_params is not None:
            raise NotImplementedError("FusedSGD has no mixed-precision (lp) flat mode; use FusedAdamW")
        self._schedule_lr()  # hp[0] of this step, ahead of the norm pass and the update
        if not f.params.is_cuda:
            self._step_reference()
        elif self._lw is not None:
            self._step_layerwise(_stream_ptr(f.params))
        elif self._clip is not None:
            st = _stream_ptr(f.params)
            self._clip.measure(self.hp, st)
            rc = _native.lib("plx_train").plx_sgd_flat_clip(
                f.params.data_ptr(), f.grads.data_ptr(), self.momentum_buf.data_ptr(), f.numel, f.n_decay,
                self.hp.data_ptr(), self.step.data_ptr(), self._clip.state.data_ptr(), st)
            _native.check(rc, "plx_sgd_flat_clip")
        else:
            rc = _native.lib("plx_train").plx_sgd_flat(
                f.params.data_ptr(), f.grads.data_ptr(), self.momentum_buf.data_ptr(), f.numel, f.n_decay,
                self.hp.data_ptr(), self.step.data_ptr(), _stream_ptr(f.params))
            _native.check(rc, "plx_sgd_flat")

    def _step_layerwise(self, st: int) -> None:
        """LARS: [norm pass + finalize of the clip,] the three layer-wise passes over the decay segments, and the
        plain launch (``n_decay`` 0) over the 1-D tail, all on the current stream."""
        f, lib = self.flat, _native.lib("plx_train")
        if self._clip is not None:
            self._clip.measure(self.hp, st)
        self._lw.step(self.momentum_buf, None, self.hp, self.step, self._clip, st)
        nd = f.n_decay
        if f.numel > nd:
            p, g, m = (t.data_ptr() + 4 * nd for t in (f.params, f.grads, self.momentum_buf))
            if self._clip is not None:
                _native.check(lib.plx_sgd_flat_clip(p, g, m, f.numel - nd, 0, self.hp.data_ptr(),
                                                    self.step.data_ptr(), self._clip.state.data_ptr(), st),
                              "plx_sgd_flat_clip")
            else:
                _native.check(lib.plx_sgd_flat(p, g, m, f.numel - nd, 0, self.hp.data_ptr(), self.step.data_ptr(),
                                               st), "plx_sgd_flat")

    @torch.no_grad()
    def _step_reference(self) -> None:
        f = self.flat
        lr, mom, wd, nest, damp = (float(self.hp[i]) for i in range(5))
        g = f.grads.clone()
        if self._clip is not None:
            scale = self._clip.measure_reference(self.hp)
            if scale is None:  # non-finite norm: the step is skipped, only the gradients are zeroed
                f.grads.zero_()
                return
            g.mul_(scale)  # a rounding step of its own, before weight decay (torch's order)
        g[: f.n_decay] += wd * f.params[: f.n_decay]
        if self._lw is not None:  # LARS: d = r (g + wd w) per decay segment
            tc = self.hp[6]
            for lo, hi in self._lw.spans():
                wn, gn = f.params[lo:hi].norm(), f.grads[lo:hi].mul(1.0 if self._clip is None else scale).norm()
                if float(wn) > 0.0 and float(gn) > 0.0:
                    g[lo:hi] *= tc * wn / (gn + wd * wn + 1e-8)
        if int(self.step.item()) == 0:
            self.momentum_buf.copy_(g)
        else:
            self.momentum_buf.mul_(mom).add_(g, alpha=1.0 - damp)
        d = g + mom * self.momentum_buf if nest else self.momentum_buf
        f.params.sub_(lr * d)
        f.grads.zero_()

    def state_buffers(self) -> Dict[str, torch.Tensor]:
        return {"momentum": self.momentum_buf}


class FusedAdamW(_Clipping, _Layerwise, _Scheduled):
    """AdamW with decoupled weight decay on the decay segment only; with ``lamb=True`` LAMB: the moments and bias
    correction are AdamW's, u = m^/(sqrt(v^) + eps) + wd w, and per decay segment r = |w| / |u| (1 unless both norms
    are positive) scales the step, w -= lr r u."""

    HP = ("lr", "beta1", "beta2", "eps", "weight_decay")

    def __init__(self, flat: FlatParams, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, step_counter: Optional[torch.Tensor] = None,
                 max_grad_norm: Optional[float] = None, lr_schedule: Optional[str] = None, lamb: bool = False,
                 muon=None, muon_lr: float = 0.02, muon_momentum: float = 0.95):
        """``muon``: names of weight matrices that get Muon instead of AdamW for the optimizer's lifetime:
        m <- mu m + g, u = g + mu m (Nesterov), O = five Newton-Schulz iterations on u / (|u| + 1e-7),
        w <- w (1 - lr_m wd) - lr_m sqrt(max(1, rows / cols)) O, with lr_m = ``muon_lr`` x the LR schedule's factor.
        The momentum lives in ``exp_avg``; ``muon_lr`` / ``muon_momentum`` are device hyper-parameters (hp slots
        6, 7).  Every other element keeps AdamW.  Not with ``lamb`` or the per-bucket updates.  None: nothing exists.
        ``lamb``: LAMB on the decay segments for the optimizer's lifetime (fp32 and lp mode; no hyper-parameter
        of its own); it excludes the per-bucket updates like clipping does.
        ``max_grad_norm``: a number enables global-norm gradient clipping for the optimizer's lifetime (a device
        hyper-parameter like the others; 0 = measure the norm, no limit); None: no clipping at all.  Clipping needs
        the whole gradient before any update, so it excludes the per-bucket updates (``step_range_``,
        ``FlatDDP(optimizer=...)``).
        ``lr_schedule``: a kind name (ops/lr_schedule.py KINDS) enables the device-resident LR schedule for the
        optimizer's lifetime, ``lr`` being its base LR; None: constant ``lr``, no schedule at all.  Per-bucket
        updates are supported: the step's first ``step_range_`` evaluates the schedule on its stream."""
        self.flat = flat
        dev = flat.device
        self.exp_avg = torch.zeros_like(flat.params)
        self.exp_avg_sq = torch.zeros_like(flat.params)
        self.hp = torch.zeros(8, dtype=torch.float32, device=dev)
        self.step = step_counter if step_counter is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        self._init_clip(flat, max_grad_norm)
        if lamb:
            self._init_layerwise(flat, _LayerNorms.LAMB if flat.lp_params is None else _LayerNorms.LAMB_LP)
        mu = {}
        if muon is not None:
            if lamb:
                raise ValueError("muon= and lamb=True both claim the weight matrices' update: choose one")
            self._mu = _MuonSegments(flat, muon)
            if len(self.HP) == _GradClip.SLOT:
                self.HP = self.HP + ("_slot5",)  # no clipping: slot 5 stays 0, as under _init_layerwise
            self.HP = self.HP + ("muon_lr", "muon_momentum")  # this instance only: hp slots 6 and 7
            mu = {"muon_lr": muon_lr, "muon_momentum": muon_momentum}
        sched = self._init_sched(flat, lr_schedule)
        self.set_hparams(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay,
                         **({"max_grad_norm": max_grad_norm} if self.clipping else {}), **mu, **sched)

    def set_hparams(self, **hp) -> None:
        self._set_hparams("AdamW", hp)

    def reset_state(self) -> None:
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        if self._clip is not None:
            self._clip.reset()

    def shard_state(self, numel: int) -> None:
        """ZeRO-1 (FlatDDP(shard_optimizer=True)): keep the moments only for the ``numel`` flat elements this rank
        updates, packed; every update then names its range's offset in that packed state (``step_range_(state_off=)``).
        The full-size moments are released."""
        self._no_ranges("sharded state")
        dev = self.flat.device
        self.exp_avg = torch.zeros(numel, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(numel, dtype=torch.float32, device=dev)
        self.sharded = True

    sharded = False

    def step_(self) -> None:
        f = self.flat
        f.grads_consumed()  # every kernel below zeroes the gradients it reads
        if self._sched is not None:
            self._sched.queued = False  # the next step's first step_range_ evaluates the schedule again
        if self.in_backward:
            return  # every bucket was already updated (FlatDDP.finish joined the optimizer stream)
        if self.sharded:
            raise RuntimeError("sharded AdamW state is updated per bucket by FlatDDP; step_() alone would skip it")
        self._schedule_lr()  # hp[0] of this step, ahead of the norm pass and the update
        if not f.params.is_cuda:
            self._step_reference()
            return
        lib = _native.lib("plx_train")
        st = _stream_ptr(f.params)
        if self._lw is not None:
            self._step_layerwise(lib, st)
            return
        if self._mu is not None:
            self._step_muon(lib, st)
            return
        if self._clip is not None:
            self._step_clipped(lib, st)
            return
        if f.lp_params is None:
            rc = lib.plx_adamw_flat(
                f.params.data_ptr(), f.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                f.numel, f.n_decay, self.hp.data_ptr(), self.step.data_ptr(), st)
            _native.check(rc, "plx_adamw_flat")
            return
        # lp mode: bf16 decay segment (master fp32 + bf16 model copy) and the fp32 tail
        nd = f.n_decay
        if nd:
            _native.check(lib.plx_adamw_mixed(
                f.params.data_ptr(), f.lp_grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                f.lp_params.data_ptr(), nd, 1, self.hp.data_ptr(), self.step.data_ptr(), st), "plx_adamw_mixed")
        if f.numel > nd:
            off = nd * 4
            _native.check(lib.plx_adamw_flat(
                f.params.data_ptr() + off, f.grads.data_ptr(), self.exp_avg.data_ptr() + off,
                self.exp_avg_sq.data_ptr() + off, f.numel - nd, 0, self.hp.data_ptr(), self.step.data_ptr(), st),
                "plx_adamw_flat")

    def _step_clipped(self, lib, st: int) -> None:
        """Norm pass + finalize + the ``*_clip`` launches of :meth:`step_`'s ranges, all on the current stream."""
        f, clip = self.flat, self._clip
        clip.measure(self.hp, st)
        hp, step, state = self.hp.data_ptr(), self.step.data_ptr(), clip.state.data_ptr()
        if f.lp_params is None:
            _native.check(lib.plx_adamw_flat_clip(
                f.params.data_ptr(), f.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                f.numel, f.n_decay, hp, step, state, st), "plx_adamw_flat_clip")
            return
        nd = f.n_decay
        if nd:
            _native.check(lib.plx_adamw_mixed_clip(
                f.params.data_ptr(), f.lp_grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                f.lp_params.data_ptr(), nd, 1, hp, step, state, st), "plx_adamw_mixed_clip")
        if f.numel > nd:
            off = nd * 4
            _native.check(lib.plx_adamw_flat_clip(
                f.params.data_ptr() + off, f.grads.data_ptr(), self.exp_avg.data_ptr() + off,
                self.exp_avg_sq.data_ptr() + off, f.numel - nd, 0, hp, step, state, st), "plx_adamw_flat_clip")

    def _step_layerwise(self, lib, st: int) -> None:
        """LAMB: [norm pass + finalize of the clip,] the three layer-wise passes over the decay segments, and the
        plain AdamW launch (``n_decay`` 0) over the 1-D tail, all on the current stream."""
        f, clip = self.flat, self._clip
        if clip is not None:
            clip.measure(self.hp, st)
        self._lw.step(self.exp_avg, self.exp_avg_sq, self.hp, self.step, clip, st)
        nd = f.n_decay
        if f.numel > nd:
            off = nd * 4
            args = (f.params.data_ptr() + off, f.grads.data_ptr() + (0 if f.lp_params is not None else off),
                    self.exp_avg.data_ptr() + off, self.exp_avg_sq.data_ptr() + off, f.numel - nd, 0,
                    self.hp.data_ptr(), self.step.data_ptr())
            if clip is not None:
                _native.check(lib.plx_adamw_flat_clip(*args, clip.state.data_ptr(), st), "plx_adamw_flat_clip")
            else:
                _native.check(lib.plx_adamw_flat(*args, st), "plx_adamw_flat")

    def _step_muon(self, lib, st: int) -> None:
        """[Norm pass + finalize of the clip,] Muon over its matrices (ops/muon.py MuonPlan.step) and the AdamW
        launches, plain or clipped, over the runs between them, all on the current stream."""
        f, clip = self.flat, self._clip
        side_stream.join(f.device)  # the momentum pass reads gradient slots the side-stream GEMMs write
        if clip is not None:
            clip.measure(self.hp, st)
        state = clip.state if clip is not None else None
        self._mu.plan.step(f, self.exp_avg, self.hp, self._sched.sched if self._sched is not None else None, state, st)
        hp, step, nd = self.hp.data_ptr(), self.step.data_ptr(), f.n_decay
        tail = (state.data_ptr(), st) if clip is not None else (st,)
        for lo, hi in self._mu.runs:
            p, m, v = (t.data_ptr() + 4 * lo for t in (f.params, self.exp_avg, self.exp_avg_sq))
            if f.lp_params is not None and hi <= nd:
                fn = lib.plx_adamw_mixed_clip if clip is not None else lib.plx_adamw_mixed
                _native.check(fn(p, f.lp_grads.data_ptr() + 2 * lo, m, v, f.lp_params.data_ptr() + 2 * lo, hi - lo, 1,
                                 hp, step, *tail), "plx_adamw_mixed")
            else:
                fn = lib.plx_adamw_flat_clip if clip is not None else lib.plx_adamw_flat
                _native.check(fn(p, f.grads.data_ptr() + 4 * (lo - f.grad_base), m, v, hi - lo,
                                 max(0, min(hi, nd) - lo), hp, step, *tail), "plx_adamw_flat")

    def step_range_(self, lo: int, hi: int, stream: Optional[int] = None, state_off: Optional[int] = None) -> None:
        """AdamW over flat elements [lo, hi) on ``stream`` (a FlatDDP bucket: 4-aligned, and in lp mode entirely
        inside the bf16 decay segment or entirely inside the fp32 tail).  The same per-element update as
        :meth:`step_`; weight decay applies to the elements below ``n_decay``; the range's gradients are zeroed.
        ``state_off``: where the range's moments start in the packed (sharded) state; default ``lo``."""
        if self._clip is not None:
            raise ValueError("max_grad_norm needs the whole gradient before any update: a clipping optimizer has no "
                             "per-range step (step_range_, FlatDDP(optimizer=...), ZeRO-1)")
        self._no_ranges("per-range step")
        f = self.flat
        so = lo if state_off is None else state_off
        if self._sched is not None and not self._sched.queued:
            # the step's first range: every range of a step runs on one stream (FlatDDP's optimizer stream), so the
            # launch boundary orders hp[0] ahead of all of them; step_() re-arms the flag
            self._schedule_lr(stream)
            self._sched.queued = True
        if not f.params.is_cuda:
            self._step_reference_range(lo, hi, so)
            return
        lib = _native.lib("plx_train")
        st = stream if stream is not None else _stream_ptr(f.params)
        nd, n = f.n_decay, hi - lo
        p, m, v = f.params.data_ptr() + 4 * lo, self.exp_avg.data_ptr() + 4 * so, self.exp_avg_sq.data_ptr() + 4 * so
        if f.lp_params is None:
            rc = lib.plx_adamw_flat(p, f.grads.data_ptr() + 4 * lo, m, v, n, max(0, min(hi, nd) - lo),
                                    self.hp.data_ptr(), self.step.data_ptr(), st)
            _native.check(rc, "plx_adamw_flat")
        elif hi <= nd:
            rc = lib.plx_adamw_mixed(p, f.lp_grads.data_ptr() + 2 * lo, m, v, f.lp_params.data_ptr() + 2 * lo, n, 1,
                                     self.hp.data_ptr(), self.step.data_ptr(), st)
            _native.check(rc, "plx_adamw_mixed")
        elif lo >= nd:
            rc = lib.plx_adamw_flat(p, f.grads.data_ptr() + 4 * (lo - nd), m, v, n, 0, self.hp.data_ptr(),
                                    self.step.data_ptr(), st)
            _native.check(rc, "plx_adamw_flat")
        else:
            raise ValueError(f"range [{lo}, {hi}) straddles the bf16/fp32 boundary at {nd}")

    @torch.no_grad()
    def _step_reference(self, lo: int = 0, hi: Optional[int] = None) -> None:
        f = self.flat
        if lo != 0 or (hi is not None and hi != f.numel):
            self._step_reference_range(lo, f.numel if hi is None else hi)
            return
        lr, b1, b2, eps, wd = (float(self.hp[i]) for i in range(5))
        t = int(self.step.item()) + 1
        g = f.grads if f.lp_grads is None else torch.cat([f.lp_grads.float(), f.grads])
        if self._clip is not None:
            scale = self._clip.measure_reference(self.hp)
            if scale is None:  # non-finite norm: the step is skipped, only the gradients are zeroed
                f.zero_grads()
                return
            g = g * scale  # a rounding step of its own, before the moments
        if self._mu is not None:  # the Muon matrices sit AdamW's update out: their state is put back below
            held = [(lo, hi, shape, f.params[lo:hi].clone(), self.exp_avg[lo:hi].clone(), g[lo:hi].clone())
                    for lo, hi, shape in self._mu.spans()]
        nd = f.n_decay if self._lw is None else 0  # LAMB: the decay term is part of u
        f.params[:nd].mul_(1.0 - lr * wd)
        self.exp_avg.mul_(b1).add_(g, alpha=1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        denom = (self.exp_avg_sq.sqrt() / bc2 ** 0.5).add_(eps)
        if self._lw is None:
            f.params.addcdiv_(self.exp_avg, denom, value=-lr / bc1)
        else:  # LAMB: w -= lr r u per decay segment (the padding is not touched), plain AdamW on the 1-D tail
            u = self.exp_avg / bc1 / denom
            for lo, hi in self._lw.spans():
                w = f.params[lo:hi]
                us = u[lo:hi] + wd * w
                wn, un = w.norm(), us.norm()
                r = wn / un if float(wn) > 0.0 and float(un) > 0.0 else 1.0
                w.sub_(lr * r * us)
            f.params[f.n_decay:].sub_(lr * u[f.n_decay:])
        if self._mu is not None:
            lr_m, mu = self.hp[_MuonSegments.LR], self.hp[_MuonSegments.MOMENTUM]
            if self._sched is not None and float(self._sched.sched[0]) > 0.0:
                lr_m = lr_m * (self.hp[0] / self._sched.sched[0])
            for lo, hi, shape, w, m, gm in held:
                m.mul_(mu).add_(gm)
                o = _muon.newton_schulz_reference((gm + mu * m).view(shape)).reshape(-1).float()
                self.exp_avg[lo:hi] = m
                self.exp_avg_sq[lo:hi] = 0.0
                f.params[lo:hi] = w * (1.0 - lr_m * wd) - lr_m * max(1.0, shape[0] / shape[1]) ** 0.5 * o
        f.zero_grads()
        f.sync_lp()

    @torch.no_grad()
    def _step_reference_range(self, lo: int, hi: int, so: Optional[int] = None) -> None:
        """The reference update restricted to [lo, hi) (CPU).  It runs inside the backward (FlatDDP optimizer mode),
        so it writes through ``.data``: the parameters are views of the flat buffers and share their autograd version
        counter, which an in-place op on any slice would bump under the tensors other layers saved for backward (the
        native kernels write through pointers and never touch it)."""
        f = self.flat
        lr, b1, b2, eps, wd = (float(self.hp[i]) for i in range(5))
        t = int(self.step.item()) + 1
        so = lo if so is None else so
        g = f.grad_view(lo, hi).data
        p, m, v = f.params.data[lo:hi], self.exp_avg[so:so + hi - lo], self.exp_avg_sq[so:so + hi - lo]
        nd = max(0, min(hi, f.n_decay) - lo)
        if nd:
            p[:nd].mul_(1.0 - lr * wd)
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        p.addcdiv_(m, (v.sqrt() / bc2 ** 0.5).add_(eps), value=-lr / bc1)
        g.zero_()
        if f.lp_params is not None and hi <= f.n_decay:
            f.lp_params.data[lo:hi].copy_(p)

    def state_buffers(self) -> Dict[str, torch.Tensor]:
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
