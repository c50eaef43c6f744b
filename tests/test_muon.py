"""Muon in ``FusedAdamW(muon=)`` on the CPU: the Newton-Schulz twin (ops/muon.py) against a closed form, the refusals,
the hyper-parameter slots and the ``muon: true`` plumbing of the gpt2 programs.  Also the inputs and the tiny model the
GPU tests (tests/test_gpu_muon.py) share, and the twin's own float32 / float64 spread that sets their margin."""
import pytest
import torch
import torch.nn as nn

from polyaxon_amd.ops.flat import FlatParams
from polyaxon_amd.ops.muon import COEF, ITERS, newton_schulz_reference
from polyaxon_amd.ops.optim import FusedAdamW

# ragged tile edges in both dimensions, more than one K step, an off-diagonal (mirrored) tile, the tall orientation
SHAPES = [(64, 64), (96, 160), (136, 264), (160, 96)]
SEEDS = (0, 1, 2)
# max |twin(float64) - twin(float32)| over SHAPES x SEEDS, measured by test_twin_spread below (profiles/muon.md)
TWIN_SPREAD = 6.84e-3


def ns_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(r, c, generator=gen).bfloat16() for r, c in SHAPES]


class TinyLM(nn.Module):
    """tiny_llama-sized parameters (d_model 64, d_ff 128): three hidden matrices (square, tall, wide) between an
    embedding and a head that stay on AdamW, and two 1-D norm weights."""

    MUON = ("wq.weight", "up.weight", "down.weight")

    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(256, 64)
        self.wq, self.up, self.down = nn.Linear(64, 64, bias=False), nn.Linear(64, 128, bias=False), nn.Linear(
            128, 64, bias=False)
        self.n1, self.n2 = nn.LayerNorm(64), nn.LayerNorm(64)
        self.head = nn.Linear(64, 256, bias=False)


def tiny_optimizer(device, lp, clip, muon=TinyLM.MUON, **kw):
    torch.manual_seed(3)
    flat = FlatParams(TinyLM(), device, lp_dtype=torch.bfloat16 if lp else None)
    opt = FusedAdamW(flat, lr=1e-3, weight_decay=0.1, muon=muon, max_grad_norm=0.5 if clip else None, **kw)
    return flat, opt


def load_grads(flat, k):
    gen = torch.Generator().manual_seed(100 + k)
    for buf in (flat.grads, flat.lp_grads):
        if buf is not None:
            buf.copy_(torch.randn(buf.numel(), generator=gen).mul(0.02).to(buf.dtype))


@pytest.mark.parametrize("shape", [(64, 128), (128, 64)])
def test_twin_without_rounding_is_the_quintic_of_the_singular_values(shape):
    a, b, c = COEF
    u = torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    U, S, Vh = torch.linalg.svd(u / (u.norm() + 1e-7), full_matrices=False)
    for _ in range(ITERS):
        S = a * S + b * S ** 3 + c * S ** 5
    want = U @ torch.diag(S) @ Vh
    got = newton_schulz_reference(u, rounding=False)
    assert float((got - want).norm() / want.norm()) <= 1e-10


def test_twin_spread():
    spread = max(float((newton_schulz_reference(u) - newton_schulz_reference(u, dtype=torch.float32).double()).abs().max())
                 for seed in SEEDS for u in ns_inputs(seed))
    print(f"twin float64 vs float32: max abs {spread:.6e}")
    assert spread <= TWIN_SPREAD


def test_refusals():
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="lamb"):
        tiny_optimizer(cpu, False, False, lamb=True)
    for bad in ("n1.weight", "nope"):
        with pytest.raises(ValueError, match=bad):
            tiny_optimizer(cpu, False, False, muon=(bad,))
    flat = FlatParams(nn.Linear(12, 64, bias=False), cpu)
    with pytest.raises(ValueError, match="weight"):
        FusedAdamW(flat, muon=("weight",))
    flat, opt = tiny_optimizer(cpu, False, False)
    with pytest.raises(ValueError, match="Muon"):
        opt.step_range_(0, 64)
    with pytest.raises(ValueError, match="Muon"):
        opt.shard_state(64)
    with pytest.raises(ValueError, match="Muon"):
        opt.in_backward = True


@pytest.mark.parametrize("clip", [False, True])
def test_hyper_parameter_slots(clip):
    _, opt = tiny_optimizer(torch.device("cpu"), False, clip, muon_lr=0.03, muon_momentum=0.9, lr_schedule="cosine")
    assert opt.hp.tolist() == pytest.approx([1e-3, 0.9, 0.999, 1e-8, 0.1, 0.5 if clip else 0.0, 0.03, 0.9])
    opt.set_hparams(muon_lr=0.05)
    assert float(opt.hp[6]) == pytest.approx(0.05) and float(opt.hp[7]) == pytest.approx(0.9)
    _, plain = tiny_optimizer(torch.device("cpu"), False, clip, muon=None)
    assert "muon_lr" not in plain.HP and plain._mu is None


def test_only_the_named_matrices_leave_adamw():
    cpu = torch.device("cpu")
    (flat, opt), (ref_flat, ref) = tiny_optimizer(cpu, False, False), tiny_optimizer(cpu, False, False, muon=None)
    for k in range(2):
        for f, o in ((flat, opt), (ref_flat, ref)):
            load_grads(f, k)
            o.step_()
    inside = torch.zeros(flat.numel, dtype=torch.bool)
    for lo, hi, shape in opt._mu.spans():
        inside[lo:hi] = True
        step = (flat.params[lo:hi] - ref_flat.params[lo:hi]).view(shape)
        assert float(step.abs().max()) > 1e-3  # an orthogonalised step of muon_lr 0.02, not AdamW's of lr 1e-3
        assert not bool(opt.exp_avg_sq[lo:hi].any())
    for a, b in ((flat.params, ref_flat.params), (opt.exp_avg, ref.exp_avg), (opt.exp_avg_sq, ref.exp_avg_sq)):
        assert torch.equal(a[~inside], b[~inside])
    assert not bool(flat.grads.any())


def test_gpt2_program_takes_muon():
    from polyaxon_amd.models.transformer import muon_parameter_names
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("gpt2_tiny", {"muon": True}, torch.device("cpu"))
    opt, model = prog.executor.opt, prog.executor.model
    names = muon_parameter_names(model)
    assert len(names) == 4 * len(model.blocks) and {s.name for s in opt._mu.segs} == set(names)
    assert all(n.startswith("blocks.") for n in names)  # the embeddings are owned by no block
    assert {"muon_lr", "muon_momentum"} <= set(prog.hp_keys)
    prog.executor.set_hparams(lr=1e-3, muon_lr=0.01, muon_momentum=0.9)
    assert float(opt.hp[6]) == pytest.approx(0.01)
    with pytest.raises(ValueError, match="layerwise"):
        build_program("gpt2_tiny", {"muon": True, "layerwise": True}, torch.device("cpu"))
