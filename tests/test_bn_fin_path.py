"""Which kernels a BatchNorm reduce + finalize with a counter array runs (csrc/bn_kernels.hip ``plx_bn_fin_path``, host
only): the single-workgroup kernels for at most T = 512 partial rows, the ticket kernels above, and the ticket kernels
throughout when ``plx_bn_set_fin_single(0)`` (``PLX_BN_FIN_SINGLE=0``) selects them."""
import pytest

T = 512
TICKET, SINGLE = 1, 2

# (partial rows, channels) of ResNet-50's BatchNorms at batch 256 whose partials come from a GEMM epilogue over
# 128-row tiles: 7x7 (layer 4), 14x14 (layer 3 and 4.0.bn1), 28x28 (layer 2 and 3.0.bn1), 56x56 (layer 1 and 2.0.bn1)
RESNET50 = [(98, 512), (98, 2048), (392, 256), (392, 512), (392, 1024), (1568, 128), (1568, 256), (1568, 512),
            (6272, 64), (6272, 128), (6272, 256)]


@pytest.fixture
def lib():
    from polyaxon_amd.ops import _native

    handle = _native.lib("plx_bn")
    handle.plx_bn_set_fin_single(1)
    yield handle
    handle.plx_bn_set_fin_single(1)


def test_resnet50_pairs(lib):
    for nblk, c in RESNET50:
        assert lib.plx_bn_fin_path(nblk, c) == (SINGLE if nblk <= T else TICKET), (nblk, c)
    assert sum(lib.plx_bn_fin_path(n, c) == SINGLE for n, c in RESNET50) == 5


def test_threshold_is_exact(lib):
    for c in (8, 64, 128, 1024, 2048):
        assert [lib.plx_bn_fin_path(n, c) for n in (1, 2, 64, 65, T - 1, T, T + 1, 784, 1600)] == \
            [SINGLE] * 6 + [TICKET] * 3


def test_switch_flips_it(lib):
    lib.plx_bn_set_fin_single(0)
    assert all(lib.plx_bn_fin_path(n, c) == TICKET for n, c in RESNET50)
    assert lib.plx_bn_fin_path(1, 8) == TICKET
    lib.plx_bn_set_fin_single(1)
    assert lib.plx_bn_fin_path(98, 2048) == SINGLE


def test_invalid_calls(lib):
    assert lib.plx_bn_fin_path(0, 64) == -1
    assert lib.plx_bn_fin_path(98, 0) == -1
    assert lib.plx_bn_fin_path(98, 12) == -1   # not a multiple of 8
    assert lib.plx_bn_fin_path(98, 24) == -1   # C / 8 not a power of two
    # the single kernels address the partials with 32-bit byte offsets: [2][nblk][C] floats stay below 2 GiB
    assert lib.plx_bn_fin_path(T, 1 << 19) == TICKET and lib.plx_bn_fin_path(T, 1 << 18) == SINGLE
