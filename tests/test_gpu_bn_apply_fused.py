"""bn3's apply + residual + ReLU produced inside the next block's conv1 forward GEMM (csrc/conv_gemm.hip
plx_gemm_nt_bnapply, ops.conv1x1.PendingApply) vs the two kernels it replaces: the same arithmetic in the same order on
the same tiles, so everything is compared bit for bit."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (M, K, N), each with a ragged tail: two 256-row tiles | two 128-row tiles | a single K stage (prologue only) |
# exactly two stages (the buffer swap)
SHAPES = [(300, 256, 64), (200, 512, 128), (40, 64, 64), (130, 128, 128)]
GUARD = 0x7B7B   # bf16 bit pattern of the guard rows behind out
MGUARD = 0xA5    # the guard bytes behind the mask
PAD = 8          # guard rows


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(m: int, k: int, n: int, with_rsb: bool):
    """Inputs of one case and the two-kernel reference (plx_bn_apply_res_relu, then plx_gemm_nt with stats), computed
    once and shared read-only."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import _stream
    from polyaxon_amd.ops.conv1x1 import gemm_nt, nt_stats_rows

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1000 * m + k + n + int(with_rsb))
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    # zero-mean x and residual, positive scales, small biases: the sums are symmetric about ~0, half of them negative
    x, res = rnd(m, k).to(torch.bfloat16), rnd(m, k).to(torch.bfloat16)
    sb = torch.cat([torch.rand(k, device=dev, generator=gen) + 0.5, 0.2 * rnd(k)]).contiguous()
    rsb = torch.cat([torch.rand(k, device=dev, generator=gen) + 0.5, 0.2 * rnd(k)]).contiguous() if with_rsb else None
    w = (rnd(n, k) / k ** 0.5).to(torch.bfloat16)
    out = torch.empty(m, k, dtype=torch.bfloat16, device=dev)
    mask = torch.empty(m * k // 8, dtype=torch.uint8, device=dev)
    rc = _native.lib("plx_bn").plx_bn_apply_res_relu(x.data_ptr(), res.data_ptr(), out.data_ptr(), m, k, sb.data_ptr(),
                                                     mask.data_ptr(), rsb.data_ptr() if with_rsb else None, _stream())
    assert rc == 0
    nblk = -(-m // nt_stats_rows(n))
    stats = torch.full((2, nblk, n), float("nan"), device=dev)
    y = gemm_nt(out, w, stats=stats)
    torch.cuda.synchronize()
    # the standalone pass is what its definition says (fp32 expression, ReLU, one rounding; mask bit = value > 0)
    rs = res.float() * rsb[:k] + rsb[k:] if with_rsb else res.float()
    v = torch.relu(torch.addcmul(sb[k:], x.float(), sb[:k]) + rs)
    assert float((out.float() - v).abs().max()) <= 2.0 ** -8 * float(v.abs().max())
    keep = (mask.view(-1, 1) >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1
    assert torch.equal(keep.view(m, k).bool(), out > 0)
    frac = float((out > 0).float().mean())
    print(f"M{m} K{k} N{n} rsb={with_rsb}: {frac:.3f} of the sums positive")
    assert 0.35 < frac < 0.65, frac
    return dict(x=x, res=res, sb=sb, rsb=rsb, w=w, out=out, mask=mask, y=y, stats=stats, nblk=nblk)


@pytest.mark.parametrize("with_rsb", [False, True], ids=["plain", "rsb"])
@pytest.mark.parametrize("m,k,n", SHAPES)
def test_fused_kernel_is_bitwise_the_two_kernels(cuda, m, k, n, with_rsb):
    """out, mask, y and the stats partials of the fused launch equal the apply pass + plx_gemm_nt bit for bit (the
    tiles are plx_gemm_nt's, so the partials keep their layout and summation order), nothing is written past row M
    (guard rows behind out, guard bytes behind the mask, guard rows behind y), and a second run repeats the first."""
    from polyaxon_amd.ops.conv1x1 import gemm_nt_bnapply

    c = _case(m, k, n, with_rsb)
    dev = c["x"].device
    runs = []
    for _ in range(2):
        out_buf = torch.full((m + PAD, k), GUARD, dtype=torch.int16, device=dev).view(torch.bfloat16)
        mask_buf = torch.full(((m + PAD) * k // 8,), MGUARD, dtype=torch.uint8, device=dev)
        y_buf = torch.full((m + PAD, n), GUARD, dtype=torch.int16, device=dev).view(torch.bfloat16)
        stats = torch.full((2, c["nblk"], n), float("nan"), device=dev)
        gemm_nt_bnapply(c["x"], c["res"], c["sb"], c["rsb"], out_buf[:m], mask_buf, c["w"], y_buf[:m], stats)
        torch.cuda.synchronize()
        assert (_bits(out_buf[m:]) == GUARD).all(), "out rows past M were written"
        assert (mask_buf[m * k // 8:] == MGUARD).all(), "mask bytes past row M were written"
        assert (_bits(y_buf[m:]) == GUARD).all(), "y rows past M were written"
        runs.append((out_buf[:m], mask_buf[:m * k // 8], y_buf[:m], stats))
    out, mask, y, stats = runs[0]
    assert torch.equal(_bits(out), _bits(c["out"])), "out differs from the standalone apply pass"
    assert torch.equal(mask, c["mask"]), "mask differs from the standalone apply pass"
    assert torch.equal(_bits(y), _bits(c["y"])), "y differs from plx_gemm_nt on the applied tensor"
    assert torch.equal(stats.view(torch.int32), c["stats"].view(torch.int32)), "stats partials differ"
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two runs differ"


@pytest.fixture
def switch():
    """ops.conv1x1.set_bn_apply_fused, restored afterwards."""
    from polyaxon_amd.ops import conv1x1

    prev = conv1x1.set_bn_apply_fused(True)
    yield conv1x1.set_bn_apply_fused
    conv1x1.set_bn_apply_fused(prev)


@pytest.fixture
def det_wgrad():
    """The deterministic (slab) weight-gradient reducer, restored afterwards."""
    from polyaxon_amd.ops import _native

    lib = _native.lib("plx_conv")
    lib.plx_set_tn_atomic(0)
    yield
    lib.plx_set_tn_atomic(int(os.environ.get("PLX_WGRAD_ATOMIC", "1")))


def _count(monkeypatch, log):
    """Record every fused launch through the Python entry point: has it an rsb?"""
    from polyaxon_amd.ops import conv1x1

    real = conv1x1.gemm_nt_bnapply

    def gemm_nt_bnapply(x, res, sb, rsb, *args, **kw):
        log.append(rsb is not None)
        return real(x, res, sb, rsb, *args, **kw)
    monkeypatch.setattr(conv1x1, "gemm_nt_bnapply", gemm_nt_bnapply)


@pytest.mark.parametrize("chain", ["identity-identity", "downsample-identity"])
def test_autograd_block_chain_on_equals_off(cuda, monkeypatch, switch, det_wgrad, chain):
    """Two chained bottlenecks (widths 64 / 256, N = 2, 8x8: M = 128), the second an identity block whose conv1 takes
    the first one's pending output (with the downsample BatchNorm's rsb when the first is a downsampling block).  The
    fused launch leaves out, mask, y and the stats bit-identical and the backward is unchanged, so with the switch on
    and off the block outputs, the running statistics, dx, the BatchNorm parameter gradients and (with the
    deterministic weight-gradient reducer selected here) the conv weight gradients are all bit-identical."""
    from polyaxon_amd.models.resnet import Bottleneck, Downsample, run_blocks
    from polyaxon_amd.ops.norm import BatchNormAct

    torch.manual_seed(5)
    if chain == "identity-identity":
        cin, blocks = 256, [Bottleneck(256, 64), Bottleneck(256, 64)]
    else:
        cin, blocks = 64, [Bottleneck(64, 64, 1, Downsample(64, 256, 1)), Bottleneck(256, 64)]
    blocks = torch.nn.ModuleList(blocks).to(cuda).to(memory_format=torch.channels_last)
    bns = [mod for mod in blocks.modules() if isinstance(mod, BatchNormAct)]
    with torch.no_grad():
        for bn in bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    x = torch.randn(2, cin, 8, 8, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    g = torch.randn(2, 256, 8, 8, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    got = {}
    for on in (False, True):
        switch(on)
        for bn in bns:
            bn.reset_running_stats()
        blocks.zero_grad(set_to_none=True)
        outs, log = [], []
        hooks = [blk.register_forward_hook(lambda mod, a, out: outs.append(out)) for blk in blocks]
        with monkeypatch.context() as mp:
            _count(mp, log)
            xa = x.clone().requires_grad_()
            y = run_blocks(blocks, xa)
            assert (getattr(outs[0], "_plx_pending", None) is not None) == on
            y.backward(g)
        for h in hooks:
            h.remove()
        torch.cuda.synchronize()
        assert log == ([chain == "downsample-identity"] if on else []), log
        got[on] = dict(outs=[o.detach().clone() for o in outs], dx=xa.grad.clone(),
                       running=[t.clone() for bn in bns for t in (bn.running_mean, bn.running_var)],
                       grads={name: p.grad.clone() for name, p in blocks.named_parameters()})
    a, b = got[True], got[False]
    for i, (u, v) in enumerate(zip(a["outs"], b["outs"])):
        assert torch.equal(_bits(u), _bits(v)), f"output of block {i} differs on / off"
    assert torch.equal(_bits(a["dx"]), _bits(b["dx"])), "dx differs on / off"
    for u, v in zip(a["running"], b["running"]):
        assert torch.equal(u, v), "running statistics differ on / off"
    assert a["grads"].keys() == b["grads"].keys() and len(a["grads"]) > 0
    for name in a["grads"]:
        assert torch.equal(a["grads"][name], b["grads"][name]), f"{name}.grad differs on / off"


def _pending_bn3(cuda, defer: bool):
    """bn3 of a bottleneck on fixed inputs, deferred or not: (y, module)."""
    from polyaxon_amd.ops.norm import BatchNormAct

    torch.manual_seed(9)
    bn = BatchNormAct(256, act=True, residual=True).to(cuda)
    x = torch.randn(2, 256, 8, 8, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ident = torch.randn(2, 256, 8, 8, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return bn(x.requires_grad_(), ident, defer_res_relu=defer), bn


def test_pending_output_is_materialised_for_other_consumers(cuda, switch):
    """A pending output handed to a non-native 1x1 convolution, to a native one outside the fused GEMM's shape class,
    or to materialize() is filled by the standalone kernel first: equal to the undeferred BatchNorm bit for bit."""
    from polyaxon_amd.ops.bn_fused import materialize
    from polyaxon_amd.ops.conv1x1 import Conv1x1

    ref, _ = _pending_bn3(cuda, False)
    assert getattr(ref, "_plx_pending", None) is None
    torch.manual_seed(2)
    consumers = [Conv1x1(256, 64, native=False).to(cuda).to(torch.bfloat16), Conv1x1(256, 256).to(cuda), materialize]
    for consume in consumers:
        y, _ = _pending_bn3(cuda, True)
        p = y._plx_pending
        assert p.pending
        consume(y)
        torch.cuda.synchronize()
        assert p.state == "filled"
        assert torch.equal(_bits(y.detach()), _bits(ref.detach()))
        y.backward(torch.ones_like(y))                        # the mask is real: the backward runs
    torch.cuda.synchronize()


def test_untaken_pending_output_raises(cuda, switch):
    """Nothing filled the pending output (and its ReLU mask): the BatchNorm's backward raises instead of reading the
    mask, and a payload that was taken cannot be taken again."""
    y, _ = _pending_bn3(cuda, True)
    with pytest.raises(RuntimeError, match="PendingApply"):
        y.backward(torch.ones_like(y))
    y, _ = _pending_bn3(cuda, True)
    y._plx_pending.take()
    with pytest.raises(RuntimeError, match="PendingApply"):
        y._plx_pending.take()
    torch.cuda.synchronize()


def test_resnet50_issues_five_fused_launches(cuda, monkeypatch, switch):
    """A ResNet-50 training forward at batch 2 issues exactly 5 fused launches -- conv1 of layer1.1, layer1.2 (K 256,
    N 64) and layer2.1, layer2.2, layer2.3 (K 512, N 128), those of layer1.1 and layer2.1 with the downsample
    BatchNorm's rsb -- and its backward runs; the eval forward, and the training forward with the switch off, none."""
    from polyaxon_amd.models.resnet import resnet50

    torch.manual_seed(4)
    model = resnet50(num_classes=10, zero_init_residual=False).to(cuda).to(memory_format=torch.channels_last)
    x = torch.randn(2, 3, 64, 64, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    log = []
    _count(monkeypatch, log)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x).float(), torch.tensor([1, 7], device=cuda))
    assert log == [True, False, True, False, False], log
    loss.backward()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    del log[:]
    switch(False)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        model(x)
    switch(True)
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(x)
    torch.cuda.synchronize()
    assert log == [], log
