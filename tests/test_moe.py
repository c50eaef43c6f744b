"""The mixture-of-experts layer's routing plan, its reference path and its program params (no GPU)."""
import pytest
import torch
import torch.nn.functional as F

from polyaxon_amd.ops import moe


def test_plan_is_a_stable_sort_by_expert():
    T, k, E = 37, 2, 5
    ids = torch.randint(0, E, (T, k), generator=torch.Generator().manual_seed(0))
    ids[:, 1] = (ids[:, 0] + 1 + ids[:, 1] % (E - 1)) % E  # two different experts per token, like a top-k
    ids[ids == 3] = 4  # expert 3 stays empty
    offs, token_of, slot_of = moe.plan(ids, E)
    assert offs.dtype == token_of.dtype == slot_of.dtype == torch.int32
    assert offs[0] == 0 and offs[E] == T * k and offs[3] == offs[4]
    pairs = torch.arange(T * k)
    assert torch.equal(token_of[slot_of.reshape(-1).long()].long(), pairs // k)  # mutually inverse
    assert torch.equal(slot_of.reshape(-1).long().sort().values, pairs)
    for e in range(E):
        seg = token_of[offs[e]:offs[e + 1]].long()
        assert bool((ids[seg] == e).any(1).all())
        assert bool((seg[1:] >= seg[:-1]).all())  # token order inside a segment: the sort is stable


@pytest.mark.parametrize("act", moe.ACTS)
def test_reference_moe_of_identical_experts_is_the_dense_mlp(act):
    """float64: the gates sum to 1, so E copies of one expert give that expert's MLP"""
    T, d, ff, E = 24, 16, 32, 4
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, T // 2, d, generator=g, dtype=torch.float64)
    up = torch.randn(2 * ff if act == "swiglu" else ff, d, generator=g, dtype=torch.float64) / 4
    down = torch.randn(d, ff, generator=g, dtype=torch.float64) / 4
    router = torch.randn(E, d, generator=g, dtype=torch.float64)
    y, aux = moe.moe_mlp(x, router, up.expand(E, -1, -1), down.expand(E, -1, -1), top_k=2, act=act)
    h = F.linear(x, up)
    dense = F.linear(moe.lm_ops.swiglu_reference(h) if act == "swiglu" else F.gelu(h, approximate="tanh"), down)
    assert float((y - dense).abs().max()) < 1e-12
    assert float(aux) >= 1.0 - 1e-9  # E sum f_e p_e is 1 when balanced and larger otherwise


def test_moe_params():
    from polyaxon_amd.polyflow.programs import build_program

    for name in ("resnet_tiny", "mlp"):
        with pytest.raises(ValueError, match="moe_experts"):
            build_program(name, {"moe_experts": 4}, "cpu")
    for other in ("fp8", "muon"):
        with pytest.raises(ValueError, match=other):
            build_program("gpt2_tiny", {"moe_experts": 4, other: True}, "cpu")
    names = lambda p: [n for n, _ in build_program("gpt2_tiny", p, "cpu").executor.model.named_parameters()]  # noqa: E731
    assert names({"moe_experts": 0}) == names({})
    prog = build_program("gpt2_tiny", {"moe_experts": 4, "moe_top_k": 1}, "cpu")
    assert prog.info["moe"] == {"experts": 4, "top_k": 1, "aux_coef": 0.01}
    shapes = {n: tuple(p.shape) for n, p in prog.executor.model.named_parameters() if ".mlp." in n and "blocks.0" in n}
    assert shapes == {"blocks.0.mlp.router.weight": (4, 64), "blocks.0.mlp.up.weight": (4, 256, 64),
                      "blocks.0.mlp.down.weight": (4, 64, 256)}
    prog.executor.reset(seed=0)
    prog.executor.set_hparams(lr=1e-3)
    prog.executor.run(2)  # NLL + c * aux trains; the ring holds the NLL
    assert bool(torch.isfinite(prog.executor.ring[:2]).all())
