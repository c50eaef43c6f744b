"""Host-side contract of the edge-tile GEMM path (ops/gemm.py): shape gating and the PLX_LM_GEMM_EDGE switch.
The kernel's numerics are in tests/test_gpu_gemm_edge.py."""
import pytest
import torch

from polyaxon_amd.ops import _native, gemm


@pytest.mark.parametrize("shape,ok", [((8, 8, 8), True), ((200, 136, 72), True), ((4, 8, 8), False),
                                      ((8, 50257, 768), False), ((0, 8, 8), False)])
def test_edge_supported_truth_table(shape, ok):
    assert gemm.edge_supported(*shape) is ok


def test_switch_unset_keeps_the_dispatch(monkeypatch):
    """a non-256 shape without PLX_LM_GEMM_EDGE: hipBLASLt (-1), whatever PLX_LM_GEMM says"""
    monkeypatch.delenv("PLX_LM_GEMM_EDGE", raising=False)
    x = torch.zeros(2, 100, 72, dtype=torch.bfloat16)
    w = torch.zeros(136, 72, dtype=torch.bfloat16)
    for mode in ("auto", "1"):
        monkeypatch.setenv("PLX_LM_GEMM", mode)
        assert not gemm.edge_enabled() and not gemm.linear_supported(x, w)
        assert gemm.schedule(200, 136, 72, True, True) == -1
        assert not gemm._use_edge(200, 136, 72, True, True)
    monkeypatch.setenv("PLX_LM_GEMM_EDGE", "1")
    assert gemm.edge_enabled()
    monkeypatch.setenv("PLX_LM_GEMM", "0")  # the A/B knob still sends everything to hipBLASLt
    assert not gemm.edge_enabled()


def test_gemm_rejects_unsupported_shapes_before_any_library_load(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda name: pytest.fail(f"loaded {name}"))
    a = torch.zeros(4, 8, dtype=torch.bfloat16)
    b = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        gemm.gemm(a, b, 4, 8, 8, True, True)
    h = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError):  # no GELU epilogues on the edge kernel
        gemm.gemm(b, b, 8, 8, 8, True, True, gelu_out=h)
