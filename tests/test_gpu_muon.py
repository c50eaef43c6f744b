"""GPU tests of Muon (csrc/muon_kernels.hip behind ``FusedAdamW(muon=)``) on a real MI355X.

Single stages: every element against float64 from the same bf16 inputs.  With v = mul (coef acc + add E) the kernel's
value, S the sum of |a_k b_k| and mag = |mul| (|coef| S + |add E|): the fp32 chain of K additions and at most three
more roundings (the scalars' products, the fma) err by (K + 3) 2^-23 mag, and the one bf16 store by 2^-8 |v|.

Five iterations end to end cannot be bounded that way (a rounding flip propagates through the polynomial): the kernels
differ from the float32 twin in summation order only, so they get 4x the twin's own float64 / float32 spread on these
inputs, TWIN_SPREAD of tests/test_muon.py (profiles/muon.md)."""
import pytest
import torch

from polyaxon_amd.ops.muon import COEF, MuonPlan, newton_schulz_reference
from test_muon import SEEDS, SHAPES, TWIN_SPREAD, TinyLM, load_grads, ns_inputs, tiny_optimizer

pytestmark = pytest.mark.gpu

U, E = 2.0 ** -8, 2.0 ** -23
MARGIN = 4 * TWIN_SPREAD


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(cuda):
    offsets, at = [], 0
    for r, c in SHAPES:
        offsets.append(at)
        at += r * c
    return MuonPlan(SHAPES, offsets, cuda)


def _sym(m, gen):
    t = torch.randn(m, m, generator=gen).mul(0.25)
    return (t + t.T).bfloat16()


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("stage", [1, 2, 3])
def test_single_stage_is_inside_the_derived_bound(cuda, stage, first):
    plan, gen = _plan(cuda), torch.Generator().manual_seed(7)
    a, b, c = (float(torch.tensor(v, dtype=torch.float32)) for v in COEF)
    scales = torch.tensor([0.5, 0.3, 1.7, 0.9])
    plan.scale.copy_(scales)
    inputs = []
    for p, x in enumerate(ns_inputs(0)):
        A, B = _sym(min(x.shape), gen), _sym(min(x.shape), gen)
        plan.x(p).copy_(x), plan.a(p).copy_(A), plan.b(p).copy_(B)
        inputs.append((x.double(), A.double(), B.double()))
    plan.stage(stage, first, 0, _stream())
    torch.cuda.synchronize()
    worst = 0.0
    for p, (x, A, B) in enumerate(inputs):
        s = float(scales[p]) if first else 1.0
        xo = x.T if x.shape[0] > x.shape[1] else x  # X: m x n
        if stage == 1:
            got, acc, S, K, mul, coef, add = plan.a(p), xo @ xo.T, xo.abs() @ xo.abs().T, xo.shape[1], s * s, 1.0, 0.0
        elif stage == 2:
            got, acc, S, K, mul, coef, add = plan.b(p), A @ A, A.abs() @ A.abs(), A.shape[0], 1.0, c, b * A
        else:
            got, acc, S, K, mul, coef, add = plan.x(p, 1), B @ xo, B.abs() @ xo.abs(), B.shape[0], s, 1.0, a * xo
            if x.shape[0] > x.shape[1]:
                got = got.T
        ref = mul * (coef * acc + add)
        mag = abs(mul) * (abs(coef) * S + (add.abs() if torch.is_tensor(add) else 0.0))
        bound = U * ref.abs() + (1 + U) * (K + 3) * E * mag
        got = got.double().cpu()
        worst = max(worst, float(((got - ref).abs() / bound).max()))
        if stage < 3:
            assert torch.equal(got, got.T)  # bit for bit: the mirrored tile comes from the same accumulators
    print(f"stage {stage} first={first}: max |got - ref| / bound {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("seed", SEEDS)
def test_five_iterations_match_the_twin(cuda, seed):
    plan = _plan(cuda)
    us = ns_inputs(seed)
    for p, u in enumerate(us):
        plan.x(p).copy_(u)
        plan.scale[p] = 1.0 / (u.float().norm() + 1e-7)
    out = plan.iterate(_stream())
    torch.cuda.synchronize()
    worst = max(float((plan.x(p, out).double().cpu() - newton_schulz_reference(u)).abs().max())
                for p, u in enumerate(us))
    print(f"seed {seed}: max |kernels - float64 twin| {worst:.4e} (margin {MARGIN:.4e})")
    assert worst <= MARGIN


def _two_steps(device, lp, clip, muon=TinyLM.MUON):
    flat, opt = tiny_optimizer(device, lp, clip, muon=muon)
    for k in range(2):
        load_grads(flat, k)
        opt.step_()
    return flat, opt


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("lp", [False, True])
def test_optimizer_two_steps(cuda, lp, clip):
    flat, opt = _two_steps(cuda, lp, clip)
    twin, _ = _two_steps(torch.device("cpu"), lp, clip)
    plain, plain_opt = _two_steps(cuda, lp, clip, muon=None)
    again, again_opt = _two_steps(cuda, lp, clip)
    inside = torch.zeros(flat.numel, dtype=torch.bool, device=cuda)
    for lo, hi, (r, c) in opt._mu.spans():
        inside[lo:hi] = True
        err = float((flat.params[lo:hi].cpu().double() - twin.params[lo:hi].double()).abs().max())
        allowed = 2 * 0.02 * max(1.0, r / c) ** 0.5 * MARGIN  # two steps of lr_m sqrt(max(1, r / c)) O
        print(f"lp={lp} clip={clip} {r}x{c}: |w - twin| {err:.3e} (allowed {allowed:.3e})")
        assert err <= allowed
    for a, b in ((flat.params, plain.params), (opt.exp_avg, plain_opt.exp_avg), (opt.exp_avg_sq, plain_opt.exp_avg_sq)):
        assert torch.equal(a[~inside], b[~inside])  # the AdamW ranges: what FusedAdamW without muon= computes
    for a, b in ((flat.params, again.params), (opt.exp_avg, again_opt.exp_avg)):
        assert torch.equal(a, b)
    if lp:
        assert torch.equal(flat.lp_params, flat.params[: flat.n_decay].bfloat16())
    assert not bool(flat.grads.any()) and (not lp or not bool(flat.lp_grads.any()))


def test_captured_step_takes_muon_hparams_per_trial(cuda):
    settings = [(0.02, 0.95), (0.005, 0.8)]
    eager = []
    for lr_m, mom in settings:
        flat, opt = tiny_optimizer(cuda, True, True, muon_lr=lr_m, muon_momentum=mom)
        for k in range(2):
            load_grads(flat, k)
            opt.step_()
        eager.append(flat.params.clone())
    flat, opt = tiny_optimizer(cuda, True, True)
    start = [t.clone() for t in (flat.params, flat.lp_params, opt.exp_avg, opt.exp_avg_sq)]
    lp_g, g = torch.zeros_like(flat.lp_grads), torch.zeros_like(flat.grads)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        flat.lp_grads.copy_(lp_g)
        flat.grads.copy_(g)
        opt.step_()
    for (lr_m, mom), want in zip(settings, eager):
        for t, t0 in zip((flat.params, flat.lp_params, opt.exp_avg, opt.exp_avg_sq), start):
            t.copy_(t0)
        opt.set_hparams(muon_lr=lr_m, muon_momentum=mom)
        for k in range(2):
            load_grads(flat, k)
            lp_g.copy_(flat.lp_grads), g.copy_(flat.grads)
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(flat.params, want)
