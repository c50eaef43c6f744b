"""GPU tests of the layer-wise updates (csrc/layerwise_kernels.hip: plx_lw_norms / plx_lw_ratios / plx_lw_update behind
``FusedSGD(trust_coef=)`` and ``FusedAdamW(lamb=True)``) on a real MI355X: two steps against the float64 rules of
tests/test_layerwise.py, on segments cut at the kernels' own chunk size.

Tolerance.  The inexact quantities are the two norms and the fp32 update arithmetic; the kernels sum in another order
than the CPU twin over the same elements at the same precision, so they are allowed 4x the twin's own deviation from
float64 on these inputs.  Measured (max |a - b| / max |b| per segment and buffer, largest over the six cases): the CPU
twin 3.05e-7 (LAMB, no clipping), which sets the bound at 1.22e-6; the GPU path 2.64e-7 (LAMB, no clipping)."""
import pytest
import torch

from polyaxon_amd.ops import _native
from test_layerwise import KINDS, run_two_steps

pytestmark = pytest.mark.gpu

TWIN_DEVIATION = 3.05e-7
PAD = 7.0  # what the padding after every decay segment holds before the steps, and must still hold after them


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_two_steps_match_float64_and_repeat_bitwise(cuda, kind, clip):
    c = _native.lib("plx_layerwise").plx_lw_chunk()
    worst, flat, bufs, padding = run_two_steps(kind, clip, c, cuda, pad=PAD)
    print(f"{kind} clip={clip}: GPU deviation {worst:.3e} (bound {4 * TWIN_DEVIATION:.3e})")
    assert worst <= 4 * TWIN_DEVIATION
    padding = padding.to(cuda)
    for t in [flat.params] + bufs:
        assert bool((t[padding] == PAD).all())
    if kind == "lamb_lp":
        assert torch.equal(flat.lp_params, flat.params[: flat.n_decay].bfloat16())
    _, again, bufs2, _ = run_two_steps(kind, clip, c, cuda, pad=PAD)
    for a, b in zip([flat.params] + bufs, [again.params] + bufs2):
        assert torch.equal(a, b)


def test_captured_step_takes_trust_coef_per_trial(cuda):
    """The three passes are ordinary launches over buffers allocated at construction: the mlp program's captured step
    is accepted, and ``trust_coef`` changes between replays of the same graph."""
    from polyaxon_amd.polyflow.programs import build_program

    prog = build_program("mlp", {"layerwise": True}, cuda)
    ex = prog.executor
    ex.capture(warmup=2)
    assert ex.graph is not None and not ex.graph_rejected
    graph, moved = ex.graph, []
    for tc in (0.001, 0.1):
        ex.reset(seed=1)
        ex.set_hparams(lr=0.1, momentum=0.9, weight_decay=1e-4, trust_coef=tc)
        before = ex.flat.params.clone()
        ex.run(1)
        moved.append(float((ex.flat.params - before)[: ex.flat.n_decay].norm()))
    assert ex.graph is graph
    assert moved[1] == pytest.approx(100 * moved[0], rel=1e-3)  # r is linear in trust_coef (wd |w| << |g| here)
