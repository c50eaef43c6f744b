"""Layer-wise adaptive updates (LARS: ``FusedSGD(trust_coef=)``, LAMB: ``FusedAdamW(lamb=True)``; ops/optim.py): the
fp32 CPU twins against the rules written out in float64, the r = 1 fall-backs, the skipped step, the refusals and the
``layerwise`` program param.  tests/test_gpu_layerwise.py runs the same steps through csrc/layerwise_kernels.hip.

Deviation is measured per segment and per buffer (weights, moments) over the real elements, as max |a - b| / max |b|.
An element passes through fewer than 16 fp32 roundings of values no larger than its segment's largest, so the twins
stay within 16 * 2^-24 ~ 1e-6 of float64 (measured: 1.8e-7 at most)."""
import pytest
import torch
import torch.nn as nn

from polyaxon_amd.ops.flat import FlatParams
from polyaxon_amd.ops.optim import FusedAdamW, FusedSGD

TWIN_TOL = 16 * 2.0 ** -24
KINDS = ("lars", "lamb", "lamb_lp")


class Net(nn.Module):
    """Decay segments at the places a chunked pass can go wrong (``c`` = the chunk size): under one vector with
    padding after it, one chunk exactly (all-zero weights), one chunk + 4 (all-zero gradients), two chunks + a ragged
    end, a rank-4 channels-last weight; and a tail of two 1-D parameters."""

    def __init__(self, c: int):
        super().__init__()
        shapes = {"tiny": (1, 3), "one": (c // 16, 16), "plus4": (2, c // 2 + 2), "ragged": (2, c + 501),
                  "conv": (8, 4, 3, 3), "gain": (5,), "bias": (64,)}
        for k, s in shapes.items():
            setattr(self, k, nn.Parameter(torch.zeros(s)))


def make(kind, clip, c, dev, pad=0.0):
    """``pad``: what the padding after each decay segment's real elements holds, in the weights and the moments."""
    flat = FlatParams(Net(c), torch.device(dev), lp_dtype=torch.bfloat16 if kind == "lamb_lp" else None)
    kw = {"max_grad_norm": 0.0 if clip else None}
    if kind == "lars":
        opt = FusedSGD(flat, lr=0.1, momentum=0.9, weight_decay=1e-2, nesterov=True, dampening=0.1, trust_coef=0.02,
                       **kw)
    else:
        opt = FusedAdamW(flat, lr=1e-2, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.1, lamb=True, **kw)
    real = torch.zeros(flat.numel, dtype=torch.bool)
    for s in flat.segments:
        real[s.offset: s.offset + s.numel] = True
    w = torch.randn(flat.numel, generator=torch.Generator().manual_seed(1)) * real
    one = next(s for s in flat.segments if s.name == "one")
    w[one.offset: one.offset + one.numel] = 0.0
    padding = ~real
    padding[flat.n_decay:] = False
    flat.params.copy_(w + pad * padding)
    flat.sync_lp()
    for b in opt.state_buffers().values():
        b.copy_(pad * padding)
    return flat, opt, real, padding


def set_grads(flat, real, seed):
    """Seeded gradients (bf16-representable in lp mode), zero on ``plus4`` and on the padding; returns them in fp64."""
    g = torch.randn(flat.numel, generator=torch.Generator().manual_seed(seed)) * real
    s = next(s for s in flat.segments if s.name == "plus4")
    g[s.offset: s.offset + s.numel] = 0.0
    if flat.lp_grads is not None:
        g[: flat.n_decay] = g[: flat.n_decay].bfloat16().float()
        flat.lp_grads.copy_(g[: flat.n_decay])
    flat.grads.copy_(g[flat.grad_base:])
    return g.double()


def ref_step(flat, lamb, hp, t, w, g, st, scale):
    """The issue's rules in float64 on flat tensors: ``w`` and the moments ``st`` are updated in place."""
    g = g * scale
    spans = [(s.offset, s.offset + s.numel) for s in flat.segments if s.decay]
    if not lamb:
        lr, mom, wd, nest, damp, _, tc = hp[:7]
        d = g.clone()
        for lo, hi in spans:
            wn, gn = w[lo:hi].norm(), g[lo:hi].norm()
            r = tc * wn / (gn + wd * wn + 1e-8) if wn > 0 and gn > 0 else 1.0
            d[lo:hi] = r * (g[lo:hi] + wd * w[lo:hi])
        st[0].copy_(d if t == 1 else mom * st[0] + (1 - damp) * d)
        w -= lr * (d + mom * st[0] if nest else st[0])
        return
    lr, b1, b2, eps, wd = hp[:5]
    st[0].copy_(b1 * st[0] + (1 - b1) * g)
    st[1].copy_(b2 * st[1] + (1 - b2) * g * g)
    upd = (st[0] / (1 - b1 ** t)) / ((st[1] / (1 - b2 ** t)).sqrt() + eps)
    for lo, hi in spans:
        u = upd[lo:hi] + wd * w[lo:hi]
        wn, un = w[lo:hi].norm(), u.norm()
        w[lo:hi] -= lr * (wn / un if wn > 0 and un > 0 else 1.0) * u
    w[flat.n_decay:] -= lr * upd[flat.n_decay:]


def deviation(flat, got, want):
    worst = 0.0
    for s in flat.segments:
        a, b = got[s.offset: s.offset + s.numel].double().cpu(), want[s.offset: s.offset + s.numel]
        top = float(b.abs().max())
        worst = max(worst, float((a - b).abs().max()) / top if top else float(a.abs().max()))
    return worst


def run_two_steps(kind, clip, c, dev, pad=0.0):
    """Two steps (first-step momentum rule, then the moving average; bias correction at t = 1, 2) against float64.
    Returns the largest deviation, the flat buffers, the moments and the decay segments' padding mask."""
    flat, opt, real, padding = make(kind, clip, c, dev, pad)
    bufs = list(opt.state_buffers().values())
    w64, st64 = flat.params.double().cpu(), [b.double().cpu() for b in bufs]
    worst = 0.0
    for t in (1, 2):
        g64 = set_grads(flat, real, seed=10 + t)
        if clip:  # a threshold at half the norm: the scale is about 0.5
            opt.set_hparams(max_grad_norm=0.5 * float(g64.norm()))
        opt.step_()
        opt.step += 1
        scale = opt.clip_stats()["scale"] if clip else 1.0
        ref_step(flat, kind != "lars", opt.hp.double().tolist(), t, w64, g64, st64, scale)
        worst = max([worst, deviation(flat, flat.params, w64)] + [deviation(flat, b, r) for b, r in zip(bufs, st64)])
        assert float(flat.grads.abs().max()) == 0.0
        assert flat.lp_grads is None or float(flat.lp_grads.float().abs().max()) == 0.0
    return worst, flat, bufs, padding


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_twin_matches_float64(kind, clip):
    worst, flat, _, _ = run_two_steps(kind, clip, 64, "cpu")
    print(f"{kind} clip={clip}: twin deviation {worst:.3e}")
    assert worst <= TWIN_TOL
    if flat.lp_params is not None:
        assert torch.equal(flat.lp_params, flat.params[: flat.n_decay].bfloat16())


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_skipped_step_touches_only_the_gradients(kind):
    flat, opt, real, _ = make(kind, True, 64, "cpu")
    set_grads(flat, real, seed=3)
    flat.grads[7] = float("inf")
    before = [flat.params.clone()] + [b.clone() for b in opt.state_buffers().values()]
    opt.step_()
    assert opt.clip_stats()["skipped"] == 1
    for a, b in zip(before, [flat.params] + list(opt.state_buffers().values())):
        assert torch.equal(a, b)
    assert float(flat.grads.abs().max()) == 0.0


def test_per_range_updates_are_refused():
    flat, opt, _, _ = make("lamb", False, 64, "cpu")
    with pytest.raises(ValueError, match="layer-wise"):
        opt.step_range_(0, 8)
    with pytest.raises(ValueError, match="layer-wise"):
        opt.shard_state(8)
    with pytest.raises(ValueError, match="layer-wise"):
        opt.in_backward = True
    assert not opt.in_backward and not opt.sharded


@pytest.mark.parametrize("name,clip", [("mlp", False), ("mlp", True), ("gpt2_tiny", False)])
def test_layerwise_program_param(name, clip):
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program(name, {"layerwise": True, "clip_grad": clip}, "cpu")
    opt = prog.executor.opt
    assert prog.info["layerwise"] is True and opt.layerwise
    if name == "mlp":
        assert "trust_coef" in prog.hp_keys and prog.info["warm_hparams"]["trust_coef"] > 0
        prog.executor.set_hparams(trust_coef=0.25, **({"max_grad_norm": 2.0} if clip else {}))
        assert opt.hp.tolist()[5:7] == [2.0 if clip else 0.0, 0.25]  # slot 6, whether or not clipping holds slot 5
    else:
        assert "trust_coef" not in prog.hp_keys and "trust_coef" not in opt.HP
    assert not build_program(name, {}, "cpu").executor.opt.layerwise
