"""The weight-gradient planner of csrc/conv_gemm.hip (tn_plan, tn2_plan, the slab workspace sizes) is host code: the
library loads without a GPU and the size queries make no launch.  The values pin the plans of the ResNet-50 weight
gradient classes at batch 256 and a few ragged shapes, so a change to the planner shows up here first."""
import pytest
import torch

from polyaxon_amd.ops import _native

# (M, N1, N2): plx_tn_plan_slices v1, v2 and plx_gemm_tn_workspace floats, all at 256 CUs
PLANS = [
    ((802816, 64, 64), 738, 185, 3358720),
    ((802816, 256, 64), 256, 191, 4718592),
    ((802816, 64, 256), 256, 191, 4718592),
    ((802816, 64, 576), 85, 64, 3502080),
    ((200704, 128, 1152), 28, 21, 4571136),
    ((200704, 512, 128), 64, 48, 4718592),
    ((50176, 256, 2304), 7, 5, 4128768),
    ((50176, 1024, 256), 16, 12, 4718592),
    ((12544, 512, 4608), 1, 4, 9437184),
    ((12544, 2048, 512), 4, 3, 4194304),
    ((12544, 2048, 1024), 2, 3, 6291456),
    ((3211264, 64, 256), 256, 192, 4718592),
    ((640, 64, 64), 2, 1, 8192),
    ((8192, 128, 128), 32, 32, 589824),
    ((100000, 192, 64), 83, 56, 1142784),
]


def _plan(lib, shape, cus):
    return (lib.plx_tn_plan_slices(*shape, cus, 0), lib.plx_tn_plan_slices(*shape, cus, 1),
            lib.plx_gemm_tn_workspace(*shape, cus))


def _queries(lib):
    for shape, v1, v2, ws in PLANS:
        assert _plan(lib, shape, 256) == (v1, v2, ws), shape
        assert _plan(lib, shape, 0) == (v1, v2, ws), shape      # 0 CUs: the 256-CU default
    assert _plan(lib, (100000, 192, 64), 64) == (21, 16, 282624)
    assert _plan(lib, (12544, 512, 4608), 64) == (1, 1, 2359296)
    assert lib.plx_stem_conv_wgrad_workspace(256, 224, 224, 256) == 9256960
    assert lib.plx_stem_conv_wgrad_workspace(256, 224, 224, 0) == 9256960
    assert lib.plx_stem_conv_wgrad_workspace(2, 32, 32, 256) == 49152
    assert lib.plx_conv_wgrad_workspace(256, 56, 56, 64, 64, 3, 1, 256) == 3502080
    assert lib.plx_conv_wgrad_workspace(256, 56, 56, 128, 128, 3, 2, 256) == 4571136
    assert lib.plx_conv_wgrad_workspace(2, 8, 8, 64, 64, 3, 1, 256) == 36864
    assert lib.plx_conv_wgrad_workspace(256, 56, 56, 256, 512, 1, 2, 256) == 4718592
    assert lib.plx_conv_dgrad_blocks(2, 9, 9, 64, 64, 3, 2) == 4
    assert lib.plx_conv_dgrad_blocks(256, 56, 56, 64, 64, 3, 1) == 3136


def test_wgrad_plans_and_workspaces():
    _queries(_native.lib("plx_conv"))


@pytest.mark.gpu
def test_workspace_queries_leave_the_kernel_choice_alone(cuda):
    """The size queries write no global: with the 128 KB ring selected, a weight gradient launched after them still
    runs and matches fp32."""
    from polyaxon_amd.ops.conv1x1 import gemm_tn

    lib = _native.lib("plx_conv")
    lib.plx_set_tn_v2(1, 128)
    try:
        _queries(lib)
        torch.manual_seed(1)
        m, n1, n2 = 1000, 64, 128
        a = torch.randn(m, n1, device=cuda).to(torch.bfloat16)
        b = torch.randn(m, n2, device=cuda).to(torch.bfloat16)
        out = gemm_tn(a, b)
        torch.testing.assert_close(out, a.float().t() @ b.float(), rtol=1e-3, atol=1e-3 * m ** 0.5)
    finally:
        lib.plx_set_tn_v2(1, 64)
