"""GPU tests of the device-resident learning-rate schedule (csrc/train_kernels.hip plx_lr_schedule; ops/optim.py
``lr_schedule``) on a real MI355X."""
import numpy as np
import pytest
import torch

from polyaxon_amd.ops import _native

pytestmark = pytest.mark.gpu

KINDS = ("constant", "linear", "cosine", "step", "inv_sqrt")
PAIRS = [(0, 1), (0, 2), (1, 2), (3, 10), (5, 5), (7, 4), (100, 100000)]  # (W, T), the CPU test's
FLOORS = (0.0, 0.1, 1.0)
GAMMA = 0.5
BASE = 3e-4

# |hp[0] - base x f64| <= 2e-6 x base (constant, linear, cosine, inv_sqrt): the cosine chain, the longest, has at
# most 8 fp32 roundings on magnitudes <= pi plus cosf's <= 2 ulp -- below 1e-6 of the factor -- and one more for the
# product with the base LR; the bound leaves 2x.  ``step``: gamma^k alone, relative 2e-6 (powf is within 2 ulp).
TOL = 2e-6


def _stream():
    return torch.cuda.current_stream().cuda_stream


def decay_every(T):
    """E of the ``step`` kind per (W, T) pair: gamma^k stays a normal fp32 number (k <= 99) over 0..T+5."""
    return 1 if T < 100 else 1000


def steps_of(W, T):
    """Every s over 0..T+5, one launch per step (about 4 us each: the long pair's 100006 steps take under a second
    per floor)."""
    return np.arange(T + 6)


def ref_factor(kind, s, W, T, m, gamma, E):
    """The schedule's formula in numpy float64 over an array of steps; also the mask of the exact-1 branches."""
    s = s.astype(np.float64)
    p = np.clip((s - W) / max(1, T - W), 0.0, 1.0)
    k = np.floor((s - W) / max(1, E))
    if kind == "constant":
        f, one = np.ones_like(s), np.ones_like(s, dtype=bool)
    elif kind == "linear":
        f = np.where(T <= W, 1.0, 1.0 - (1.0 - m) * p)
        one = (s == W) | (T <= W) | (m == 1.0)
    elif kind == "cosine":
        f = np.where(T <= W, 1.0, m + (1.0 - m) * 0.5 * (1.0 + np.cos(np.pi * p)))
        one = (s == W) | (T <= W) | (m == 1.0)
    elif kind == "step":
        f = np.maximum(m, gamma ** np.maximum(k, 0.0))
        one = (k == 0) | (m == 1.0)
    else:
        f = np.maximum(m, np.sqrt(max(W, 1) / (s + 1.0)))
        one = (s + 1 == max(W, 1)) | (m == 1.0)
    warm = s < W
    f = np.where(warm, (s + 1.0) / max(W, 1), f)
    one = np.where(warm, s + 1 == W, one)
    return f, one


def _sched(dev, base, kind, W, T, m, gamma=GAMMA, E=1):
    return torch.tensor([base, KINDS.index(kind), W, T, m, gamma, E, 0.0], dtype=torch.float32, device=dev)


def _evaluate(lib, sched, steps, dev):
    """One plx_lr_schedule launch per step, each reading its own counter and writing its own float."""
    st = torch.as_tensor(steps, dtype=torch.int32).to(dev)
    out = torch.full((len(steps),), float("nan"), device=dev)
    stream = _stream()
    sp, op, cp = st.data_ptr(), out.data_ptr(), sched.data_ptr()
    for i in range(len(steps)):
        rc = lib.plx_lr_schedule(cp, sp + 4 * i, op + 4 * i, stream)
        if rc:
            _native.check(rc, "plx_lr_schedule")
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matches_float64_over_the_grid(cuda, kind):
    lib = _native.lib("plx_train")
    base32 = float(torch.tensor(BASE, dtype=torch.float32))
    worst = 0.0
    for W, T in PAIRS:
        E = decay_every(T)
        steps = steps_of(W, T)
        for m in FLOORS:
            got = _evaluate(lib, _sched(cuda, BASE, kind, W, T, m, GAMMA, E), steps, cuda)
            got = got.cpu().numpy().astype(np.float64)
            want, one = ref_factor(kind, steps, W, T, m, GAMMA, E)
            assert np.isfinite(got).all(), (kind, W, T, m)
            if kind == "step":
                decay = GAMMA ** np.maximum(np.floor((steps - W) / E), 0.0)
                free = (steps >= W) & (decay > m)  # where gamma^k itself is the factor
                err = np.where(free, np.abs(got - base32 * want) / (base32 * want), np.abs(got - base32 * want) / base32)
            else:
                err = np.abs(got - base32 * want) / base32
            i = int(err.argmax())
            worst = max(worst, float(err[i]))
            assert err[i] <= TOL, (kind, W, T, m, int(steps[i]), got[i], base32 * want[i])
            # the exact-1 branches: hp[0] is bitwise base_lr
            assert (got[one] == base32).all(), (kind, W, T, m, steps[one][got[one] != base32][:5])
            if kind in ("linear", "cosine") and T > W:  # past the horizon: exactly base x fp32(m)
                at_floor = float(torch.tensor(BASE, dtype=torch.float32) * torch.tensor(m, dtype=torch.float32))
                assert (got[steps >= T] == (base32 if m == 1.0 else at_floor)).all(), (kind, W, T, m)
    print(f"plx_lr_schedule {kind}: worst error {worst:.3g} (bound {TOL:g})")


def test_kernel_writes_hp0_only(cuda):
    lib = _native.lib("plx_train")
    for kind in KINDS:
        sched = _sched(cuda, BASE, kind, 3, 10, 0.1, GAMMA, 2)
        sched[7] = -7.0  # reserved: never read into the result, never written
        hp = torch.arange(100.0, 116.0, device=cuda)  # hp and the 8 floats behind it
        step = torch.tensor([5, -9], dtype=torch.int32, device=cuda)
        s0, h0 = sched.clone(), hp.clone()
        _native.check(lib.plx_lr_schedule(sched.data_ptr(), step.data_ptr(), hp.data_ptr(), _stream()), "lr_schedule")
        torch.cuda.synchronize()
        assert torch.equal(sched, s0) and step.tolist() == [5, -9]
        assert torch.equal(hp[1:], h0[1:])
        want, _ = ref_factor(kind, np.array([5]), 3, 10, 0.1, GAMMA, 2)
        assert abs(float(hp[0]) - BASE * want[0]) <= TOL * BASE
    assert lib.plx_lr_schedule(0, step.data_ptr(), hp.data_ptr(), _stream()) != 0  # null pointers are refused
    assert lib.plx_lr_schedule(sched.data_ptr(), 0, hp.data_ptr(), _stream()) != 0
    assert lib.plx_lr_schedule(sched.data_ptr(), step.data_ptr(), 0, _stream()) != 0


# ---------------------------------------------------------------- scheduled optimizer kernels
def _run_kernel(lib, which, sched, cuda, hp_values=None):
    """6 steps of one optimizer kernel on n = 8196 (n_decay = 4096): with ``sched`` the schedule kernel runs ahead
    of every update; with ``hp_values`` hp[0] is set from the host instead.  Returns (state tensors, hp[0] per step)."""
    n, nd = 8196, 4096
    gen = torch.Generator(device=cuda).manual_seed(5)
    p = torch.randn(n, device=cuda, generator=gen)
    m = torch.zeros(n, device=cuda)
    v = torch.zeros(n, device=cuda)
    plp = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    hp = torch.tensor({"sgd": [BASE, 0.9, 1e-3, 0, 0, 0, 0, 0]}.get(which, [BASE, 0.9, 0.95, 1e-8, 0.1, 0, 0, 0]),
                      device=cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    lrs = []
    for it in range(6):
        g = torch.randn(n, device=cuda, generator=gen)
        if sched is not None:
            _native.check(lib.plx_lr_schedule(sched.data_ptr(), step.data_ptr(), hp.data_ptr(), _stream()), "sched")
        else:
            hp[0] = hp_values[it]
        lrs.append(hp[0].clone())
        if which == "sgd":
            rc = lib.plx_sgd_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), n, nd, hp.data_ptr(), step.data_ptr(),
                                  _stream())
        elif which == "adamw":
            rc = lib.plx_adamw_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, nd, hp.data_ptr(),
                                    step.data_ptr(), _stream())
        else:  # lp mode: the bf16 decay segment, then the fp32 tail
            g16 = g[:nd].to(torch.bfloat16)
            rc = lib.plx_adamw_mixed(p.data_ptr(), g16.data_ptr(), m.data_ptr(), v.data_ptr(), plp.data_ptr(), nd, 1,
                                     hp.data_ptr(), step.data_ptr(), _stream())
            _native.check(rc, "adamw_mixed")
            tail = g[nd:].clone()
            rc = lib.plx_adamw_flat(p.data_ptr() + 4 * nd, tail.data_ptr(), m.data_ptr() + 4 * nd,
                                    v.data_ptr() + 4 * nd, n - nd, 0, hp.data_ptr(), step.data_ptr(), _stream())
        _native.check(rc, which)
        step += 1
    torch.cuda.synchronize()
    return (p, m, v, plp), [float(x) for x in lrs]


@pytest.mark.parametrize("which", ["sgd", "adamw", "adamw_mixed"])
def test_scheduled_kernels_equal_host_set_lr_bitwise(cuda, which):
    lib = _native.lib("plx_train")
    sched = _sched(cuda, BASE, "cosine", 2, 6, 0.1)
    a, lrs = _run_kernel(lib, which, sched, cuda)
    want, _ = ref_factor("cosine", np.arange(6), 2, 6, 0.1, GAMMA, 1)
    assert all(abs(lr - BASE * w) <= TOL * BASE for lr, w in zip(lrs, want)) and len(set(lrs)) > 3
    b, lrs_b = _run_kernel(lib, which, None, cuda, hp_values=lrs)
    assert lrs_b == lrs
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- the captured step
def _twin_lr(base, hp, s):
    from polyaxon_amd.ops.optim import lr_factor

    f = lr_factor(hp["lr_schedule"], s, hp["warmup_steps"], hp["lr_total_steps"], hp["min_lr_ratio"],
                  hp.get("lr_decay_gamma", 0.1), hp.get("lr_decay_every", 1))
    return float(torch.tensor(base, dtype=torch.float32) * f)


def _close(lr, want, base):
    """The device LR against the CPU twin: each is within TOL x base of the fp64 curve (the kernel may contract a
    product and a sum that the twin rounds separately, and cosf is not torch.cos), so they agree to TOL x base, not
    bitwise."""
    return abs(lr - want) <= TOL * base


TRIALS = [
    ({"lr": 0.02, "momentum": 0.9, "weight_decay": 1e-4, "lr_schedule": "cosine", "warmup_steps": 2,
      "lr_total_steps": 7, "min_lr_ratio": 0.1}, 5),
    ({"lr": 0.05, "momentum": 0.9, "weight_decay": 1e-4, "lr_schedule": "step", "warmup_steps": 0,
      "lr_total_steps": 0, "min_lr_ratio": 0.0, "lr_decay_gamma": 0.5, "lr_decay_every": 2}, 6),
]


def test_one_captured_step_serves_every_schedule(cuda):
    """The mlp program's step is captured once with the schedule kernel in it; two trials with different kinds,
    warm-up and horizon replay the same graph, and each equals an eager executor given the same schedule bitwise."""
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("mlp", {"lr_schedule": True}, cuda)
    ex = prog.executor
    assert ex.use_graph and ex.opt.scheduled
    ex.capture(warmup=2)
    assert ex.graph is not None and not ex.graph_rejected
    graph = ex.graph
    eager = build_program("mlp", {"lr_schedule": True}, cuda).executor
    eager.use_graph = False
    for seed, (hp, steps) in enumerate(TRIALS):
        for e in (ex, eager):
            e.reset(seed=seed + 1)
            e.set_hparams(**hp)
            e.run(steps)
        torch.cuda.synchronize()
        assert ex.graph is graph and eager.graph is None
        lr = float(ex.current_lr())
        assert ex.current_lr().is_cuda and ex.current_lr().dim() == 0
        assert int(ex.step) == steps
        assert _close(lr, _twin_lr(hp["lr"], hp, steps - 1), hp["lr"]), (lr, _twin_lr(hp["lr"], hp, steps - 1))
        assert lr == float(eager.current_lr())
        assert torch.equal(ex.flat.params, eager.flat.params)
        assert torch.equal(ex.opt.momentum_buf, eager.opt.momentum_buf)


def test_constant_schedule_is_bitwise_the_unscheduled_step(cuda):
    from polyaxon_amd.polyflow.programs import build_program

    res = []
    for params in ({}, {"lr_schedule": True}):
        ex = build_program("mlp", params, cuda).executor
        ex.use_graph = False
        ex.reset(seed=4)
        ex.set_hparams(lr=0.03, momentum=0.9, weight_decay=1e-4)
        ex.run(4)
        torch.cuda.synchronize()
        res.append((ex.flat.params.clone(), float(ex.current_lr())))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


def test_clip_and_schedule_in_one_captured_step(cuda):
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("mlp", {"lr_schedule": "cosine", "clip_grad": True}, cuda)
    ex = prog.executor
    ex.capture(warmup=2)
    assert ex.graph is not None and not ex.graph_rejected
    hp = dict(TRIALS[0][0], max_grad_norm=1e-4)
    ex.reset(seed=1)
    ex.set_hparams(**hp)
    ex.run(4)
    st = ex.clip_stats()
    assert 0.0 < st["scale"] < 1.0 and st["scale"] == pytest.approx(1e-4 / st["grad_norm"], rel=1e-5)
    assert _close(float(ex.current_lr()), _twin_lr(hp["lr"], hp, 3), hp["lr"])


def test_snapshot_restore_continues_the_curve_on_the_device(cuda):
    from polyaxon_amd.polyflow.programs import build_program

    ex = build_program("mlp", {"lr_schedule": "cosine"}, cuda).executor
    ex.capture(warmup=2)
    hp = TRIALS[0][0]
    ex.reset(seed=2)
    ex.set_hparams(**hp)
    ex.run(3)
    ex.snapshot("k")
    first = []
    for _ in range(4):
        ex.run(1)
        first.append(float(ex.current_lr()))
    p1 = ex.flat.params.clone()
    ex.restore("k")
    second = []
    for _ in range(4):
        ex.run(1)
        second.append(float(ex.current_lr()))
    assert first == second and len(set(first)) == 4
    assert all(_close(lr, _twin_lr(hp["lr"], hp, s), hp["lr"]) for lr, s in zip(first, range(3, 7)))
    assert torch.equal(ex.flat.params, p1)
