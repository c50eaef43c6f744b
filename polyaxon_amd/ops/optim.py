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

On CPU (no native library) the same update is computed with torch ops; tests compare the two.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from polyaxon_amd.ops import _native, lr_schedule as _lrs, side_stream
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


class FusedSGD(_Clipping, _Scheduled):
    """SGD with momentum / nesterov / dampening and weight decay on the decay segment only."""

    HP = ("lr", "momentum", "weight_decay", "nesterov", "dampening")

    def __init__(self, flat: FlatParams, lr: float = 0.1, momentum: float = 0.9, weight_decay: float = 1e-4,
                 nesterov: bool = False, dampening: float = 0.0, step_counter: Optional[torch.Tensor] = None,
                 max_grad_norm: Optional[float] = None, lr_schedule: Optional[str] = None):
        """``max_grad_norm``: a number enables global-norm gradient clipping for the optimizer's lifetime (a device
        hyper-parameter like the others; 0 = measure the norm, no limit); None: no clipping at all.
        ``lr_schedule``: a kind name (ops/lr_schedule.py KINDS) enables the device-resident LR schedule for the
        optimizer's lifetime, ``lr`` being its base LR; None: constant ``lr``, no schedule at all."""
        self.flat = flat
        dev = flat.device
        self.momentum_buf = torch.zeros_like(flat.params)
        self.hp = torch.zeros(8, dtype=torch.float32, device=dev)
        # step counter shared with the metric ring: 0 right after reset() => momentum := grad
        self.step = step_counter if step_counter is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        self._init_clip(flat, max_grad_norm)
        sched = self._init_sched(flat, lr_schedule)
        self.set_hparams(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                         dampening=dampening, **({"max_grad_norm": max_grad_norm} if self.clipping else {}), **sched)

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
        if int(self.step.item()) == 0:
            self.momentum_buf.copy_(g)
        else:
            self.momentum_buf.mul_(mom).add_(g, alpha=1.0 - damp)
        d = g + mom * self.momentum_buf if nest else self.momentum_buf
        f.params.sub_(lr * d)
        f.grads.zero_()

    def state_buffers(self) -> Dict[str, torch.Tensor]:
        return {"momentum": self.momentum_buf}


class FusedAdamW(_Clipping, _Scheduled):
    HP = ("lr", "beta1", "beta2", "eps", "weight_decay")

    def __init__(self, flat: FlatParams, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, step_counter: Optional[torch.Tensor] = None,
                 max_grad_norm: Optional[float] = None, lr_schedule: Optional[str] = None):
        """``max_grad_norm``: a number enables global-norm gradient clipping for the optimizer's lifetime (a device
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
        sched = self._init_sched(flat, lr_schedule)
        self.set_hparams(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay,
                         **({"max_grad_norm": max_grad_norm} if self.clipping else {}), **sched)

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
        dev = self.flat.device
        self.exp_avg = torch.zeros(numel, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(numel, dtype=torch.float32, device=dev)
        self.sharded = True

    sharded = False

    # set by FlatDDP(optimizer=...): the update runs per gradient bucket during the backward (step_range_), and
    # step_() only closes the step's bookkeeping
    in_backward = False

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

    def step_range_(self, lo: int, hi: int, stream: Optional[int] = None, state_off: Optional[int] = None) -> None:
        """AdamW over flat elements [lo, hi) on ``stream`` (a FlatDDP bucket: 4-aligned, and in lp mode entirely
        inside the bf16 decay segment or entirely inside the fp32 tail).  The same per-element update as
        :meth:`step_`; weight decay applies to the elements below ``n_decay``; the range's gradients are zeroed.
        ``state_off``: where the range's moments start in the packed (sharded) state; default ``lo``."""
        if self._clip is not None:
            raise ValueError("max_grad_norm needs the whole gradient before any update: a clipping optimizer has no "
                             "per-range step (step_range_, FlatDDP(optimizer=...), ZeRO-1)")
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
        f.params[: f.n_decay].mul_(1.0 - lr * wd)
        self.exp_avg.mul_(b1).add_(g, alpha=1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        denom = (self.exp_avg_sq.sqrt() / bc2 ** 0.5).add_(eps)
        f.params.addcdiv_(self.exp_avg, denom, value=-lr / bc1)
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
