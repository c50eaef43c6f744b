"""BatchNorm-backward dx produced inside the consuming 1x1 data-gradient GEMM (csrc/conv_gemm.hip plx_gemm_nt_bndx,
ops.conv1x1.DxSink) vs today's two kernels (bit for bit where the issue is the same arithmetic) and vs fp32
F.batch_norm + F.conv2d autograd."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
# (M, K, N): one partial tile | one row past a 128- and a 256-row tile | two N tiles (dy written once) | longest K,
# largest coefficient table | one K stage
SHAPES = [(126, 256, 64), (257, 512, 128), (129, 1024, 256), (300, 2048, 512), (130, 64, 64)]
GUARD = 0x7B7B  # bf16 bit pattern of the guard rows behind dy and C


def _pack_bits(keep: torch.Tensor) -> torch.Tensor:
    """bool [..] -> the 1-bit mask layout of bn_apply_kernel: bit k of byte i = element 8 i + k."""
    w = 2 ** torch.arange(8, device=keep.device, dtype=torch.int32)
    return (keep.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(m: int, k: int, n: int, relu: bool):
    """Inputs of one case, the standalone BatchNorm backward (its dx and the coefficients of its real finalize) and
    the fp32 autograd reference, computed once and shared (read-only) by the tests of that case."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import _counters, _stream, bn_backward, bn_forward

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1000 * m + k + n + int(relu))
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    g, x = rnd(m, k).to(torch.bfloat16), rnd(m, k).to(torch.bfloat16)
    gamma, beta = torch.rand(k, device=dev, generator=gen) + 0.5, 0.2 * rnd(k)
    wt = (rnd(n, k) / k ** 0.5).to(torch.bfloat16)            # the dgrad's B operand; products are O(1)
    # the BatchNorm(+ReLU) whose output the data gradient C is the gradient of (the BnBwd epilogue's operands)
    xp = rnd(m, n).to(torch.bfloat16)
    gp, bp = torch.rand(n, device=dev, generator=gen) + 0.5, 0.2 * rnd(n)
    d_add = rnd(m, n).to(torch.bfloat16)                      # a second gradient added in the epilogue

    # --- native BatchNorm forward (mask, mean, invstd) and standalone backward (dx, coef)
    f32 = dict(dtype=torch.float32, device=dev)
    ws = _native.size("plx_bn", "plx_bn_workspace", m, k)
    stats = torch.empty(4 * k, **f32)
    y = torch.empty_like(x)
    mask = torch.empty(m * k // 8, dtype=torch.uint8, device=dev) if relu else None
    bn_forward(x=x, y=y, m=m, c=k, gamma=gamma, beta=beta, eps=EPS, momentum=0.1, save_mean=stats,
               save_invstd=stats[k:], scale_bias=stats[2 * k:], workspace=torch.empty(ws, **f32), mask=mask, relu=relu,
               counters=_counters(dev), stream=_stream())
    dx, coef, dgb = torch.empty_like(x), torch.empty(3 * k, **f32), torch.empty(2 * k, **f32)
    bn_backward(x=x, mask=mask, dy=g, dx=dx, m=m, c=k, gamma=gamma, save_mean=stats, save_invstd=stats[k:],
                dgamma=dgb, dbeta=dgb[k:], coef=coef, workspace=torch.empty(ws, **f32), relu=relu, accumulate=0,
                counters=_counters(dev), stream=_stream())

    # --- fp32 reference: dy = d sum(g * act(BN(x))) / dx, C = conv2d's data gradient of dy, and the gradients of the
    # previous BatchNorm's gamma / beta for the output gradient C (+ d_add) = the column sums of the partials
    xr = x.float().requires_grad_()
    yr = F.batch_norm(xr, None, None, gamma, beta, training=True, eps=EPS)
    if relu:
        yr = yr * (y.float() > 0)                             # the forward's own ReLU decisions
    (dy_ref,) = torch.autograd.grad((yr * g.float()).sum(), xr)
    h0 = torch.zeros(m, n, 1, 1, device=dev, requires_grad=True)
    (c_ref,) = torch.autograd.grad(F.conv2d(h0, wt.float().t().reshape(k, n, 1, 1)), h0, dy_ref.view(m, k, 1, 1))
    c_ref = c_ref.view(m, n)
    refs = {}
    for add in (False, True):
        xpr = xp.float().requires_grad_()
        g0, b0 = gp.clone().requires_grad_(), bp.clone().requires_grad_()
        hp = F.relu(F.batch_norm(xpr, None, None, g0, b0, training=True, eps=EPS))
        hp.backward(c_ref + d_add.float() if add else c_ref)
        refs[add] = (c_ref + d_add.float() if add else c_ref, b0.grad, g0.grad)
    with torch.no_grad():
        mean_p = xp.float().mean(0)
        invstd_p = (xp.float().var(0, unbiased=False) + EPS).rsqrt()
        mask_p = _pack_bits(hp > 0)
    torch.cuda.synchronize()
    return dict(g=g, x=x, mask=mask, coef=coef, dx=dx, wt=wt, xp=xp, mask_p=mask_p, mean_p=mean_p, invstd_p=invstd_p,
                d_add=d_add, refs=refs)


def _run(case, m, k, n, fused: bool, epilogue: bool):
    """One data gradient through the fused kernel or through today's dx pass + gemm_nt; (dy, C, partial sums)."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.conv1x1 import gemm_nt, gemm_nt_bndx, nt_stats_rows

    dev = case["g"].device
    pad = 8                                                    # guard rows: nothing may be written past row M
    dy_buf = torch.full((m + pad, k), GUARD, dtype=torch.int16, device=dev).view(torch.bfloat16)
    c_buf = torch.full((m + pad, n), GUARD, dtype=torch.int16, device=dev).view(torch.bfloat16)
    dy, out = dy_buf[:m], c_buf[:m]
    bnr = part = add = None
    if epilogue:
        nblk = -(-m // nt_stats_rows(n))
        part = torch.full((2, nblk, n), float("nan"), device=dev)
        bnr = _native.GemmBnBwdArgs(case["xp"].data_ptr(), case["mask_p"].data_ptr(), case["mean_p"].data_ptr(),
                                    case["invstd_p"].data_ptr(), part.data_ptr(), nblk, 0)
        add = case["d_add"]
    if fused:
        gemm_nt_bndx(case["g"], case["x"], case["mask"], case["coef"], dy, case["wt"], out, add=add, bnr=bnr)
    else:
        dy.copy_(case["dx"])
        gemm_nt(dy, case["wt"], out, add=add, bnr=bnr)
    torch.cuda.synchronize()
    assert (_bits(dy_buf[m:]) == GUARD).all() and (_bits(c_buf[m:]) == GUARD).all(), "rows past M were written"
    return dy, out, (part.sum(1) if part is not None else None)


@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bnbwd"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("m,k,n", SHAPES)
def test_fused_kernel_matches_two_kernel_path(cuda, m, k, n, relu, epilogue):
    """dy is the standalone dx pass bit for bit (same fp32 expression, one rounding); C and the BatchNorm-backward
    partials meet the tolerances of test_conv1x1_autograd (dx) and test_bn_backward_partials_from_dgrad_epilogue
    against fp32 F.batch_norm + F.conv2d autograd -- as does today's two-kernel path on the same inputs, so the
    tolerance is a property of the reference, not of the fused kernel; two runs are bitwise equal."""
    case = _case(m, k, n, relu)
    c_ref, dbeta_ref, dgamma_ref = case["refs"][epilogue]
    results = {}
    for fused in (False, True):
        dy, out, sums = _run(case, m, k, n, fused, epilogue)
        results[fused] = (dy, out, sums)
        name = "fused" if fused else "two-kernel"
        print(f"{name}: max |C - ref| = {float((out.float() - c_ref).abs().max()):.4g}")
        torch.testing.assert_close(out.float(), c_ref, rtol=2e-2, atol=5e-2, msg=lambda s: f"{name} C: {s}")
        if epilogue:
            for got, ref, what in ((sums[0], dbeta_ref, "sum dz"), (sums[1], dgamma_ref, "sum dz xhat")):
                print(f"{name}: max |{what} - ref| = {float((got - ref).abs().max()):.4g} of {float(ref.abs().max()):.4g}")
                torch.testing.assert_close(got, ref, rtol=1e-2, atol=1e-2 * float(ref.abs().max()),
                                           msg=lambda s: f"{name} {what}: {s}")
    assert torch.equal(_bits(results[True][0]), _bits(case["dx"])), "dy differs from the standalone dx pass"
    dy2, out2, sums2 = _run(case, m, k, n, True, epilogue)
    assert torch.equal(_bits(dy2), _bits(results[True][0])) and torch.equal(_bits(out2), _bits(results[True][1]))
    if epilogue:
        assert torch.equal(sums2, results[True][2])


def _spy(monkeypatch, log):
    """Record the gradient operand of every 1x1 data-gradient GEMM: (fused?, the A / dy tensor)."""
    from polyaxon_amd.ops import conv1x1

    nt, bndx = conv1x1.gemm_nt, conv1x1.gemm_nt_bndx

    def gemm_nt(a, b, out=None, *args, **kw):
        log.append((False, a))
        return nt(a, b, out, *args, **kw)

    def gemm_nt_bndx(g, x, mask, coef, dy, *args, **kw):
        log.append((True, dy))
        return bndx(g, x, mask, coef, dy, *args, **kw)
    monkeypatch.setattr(conv1x1, "gemm_nt", gemm_nt)
    monkeypatch.setattr(conv1x1, "gemm_nt_bndx", gemm_nt_bndx)


@pytest.fixture
def switch():
    """ops.conv1x1.set_bn_dx_fused, restored afterwards."""
    from polyaxon_amd.ops import conv1x1

    prev = conv1x1.set_bn_dx_fused(True)
    yield conv1x1.set_bn_dx_fused
    conv1x1.set_bn_dx_fused(prev)


@pytest.mark.parametrize("act,residual", [(True, True), (True, False), (False, False)],
                         ids=["relu-residual", "relu", "plain"])
def test_autograd_conv_bn_chain(cuda, monkeypatch, switch, act, residual):
    """x -> Conv1x1 (C -> 4C) -> BatchNormAct(act, residual through an armed box / none) -> sum(g * y), switch on and
    off: the conv input's gradient, the conv weight gradient, dgamma and dbeta meet the tolerances above against fp32
    autograd, and the BatchNorm-input gradient buffer is bitwise equal between on and off.  The reference BatchNorm
    reads the native convolution's stored bf16 output (gradients still flow through F.conv2d), so both sides take
    the same ReLU decisions.

    M = 32 rows (the tile edges are the kernel test's business): both native paths store the BatchNorm-input gradient
    dy in bf16, a relative error uniform in +-2^-9 (std 1.1e-3), which the fp32 reference does not have.  In the
    weight gradient it adds up over the M rows to std 1.1e-3 * rms(dy) * rms(x) * sqrt(M) with rms(dy) <= 1.8 here
    (gamma ~ 1, invstd ~ 1.7 of a kaiming-uniform 1x1 conv of unit inputs, unit g) and rms(x) = 1: 0.012, so the
    largest of the 16384 elements (4.1 sigma) is expected near 0.05 against the 0.1 allowed; at M = 189 it would be
    0.12."""
    from polyaxon_amd.ops.conv1x1 import Conv1x1, GradMailbox
    from polyaxon_amd.ops.norm import BatchNormAct

    shape, cout = (2, 64, 4, 4), 256                           # M = 32, 4 K stages
    torch.manual_seed(11)
    conv = Conv1x1(shape[1], cout).to(cuda)
    bn = BatchNormAct(cout, act=act, residual=residual).to(cuda)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    x = torch.randn(shape, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ident = (torch.randn(shape[0], cout, *shape[2:], device=cuda).to(torch.bfloat16)
             .contiguous(memory_format=torch.channels_last)) if residual else None
    g = torch.randn(shape[0], cout, *shape[2:], device=cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    got = {}
    for on in (False, True):
        switch(on)
        log = []
        with monkeypatch.context() as mp:
            _spy(mp, log)
            xa = x.clone().requires_grad_()
            box = GradMailbox()
            box.armed = residual
            yc = conv(xa)
            y = bn(yc, ident, residual_grad_box=box) if residual else bn(yc)
            del log[:]                                        # keep the backward's calls only
            y.backward(g)
        torch.cuda.synchronize()
        assert [f for f, _ in log] == [on], log
        got[on] = (y.detach().float(), yc.detach(), xa.grad.float(), conv.weight.grad.clone(), bn.weight.grad.clone(),
                   bn.bias.grad.clone(), log[0][1])
        conv.zero_grad(set_to_none=True)
        bn.zero_grad(set_to_none=True)
    assert torch.equal(_bits(got[True][6]), _bits(got[False][6])), "BatchNorm-input gradient differs on / off"
    # fp32 reference on the stored conv output
    xr = x.float().requires_grad_()
    wr = conv.weight.detach().clone().requires_grad_()
    gr, br = bn.weight.detach().clone().requires_grad_(), bn.bias.detach().clone().requires_grad_()
    yc32 = F.conv2d(xr, wr.to(torch.bfloat16).float())
    ycs = got[True][1].float() + (yc32 - yc32.detach())
    yr = F.batch_norm(ycs, None, None, gr, br, training=True, eps=bn.eps)
    if residual:
        yr = yr + ident.float()
    if act:
        yr = F.relu(yr)
    yr.backward(g.float())
    for on in (False, True):
        name = "on" if on else "off"
        y, _, dx, dw, dgamma, dbeta, _ = got[on]
        torch.testing.assert_close(y, yr.detach(), rtol=2e-2, atol=5e-2, msg=lambda s: f"{name} y: {s}")
        torch.testing.assert_close(dx, xr.grad, rtol=2e-2, atol=5e-2, msg=lambda s: f"{name} dx: {s}")
        torch.testing.assert_close(dw, wr.grad, rtol=2e-2, atol=0.1, msg=lambda s: f"{name} dw: {s}")
        for a, r, what in ((dgamma, gr.grad, "dgamma"), (dbeta, br.grad, "dbeta")):
            torch.testing.assert_close(a, r, rtol=1e-2, atol=1e-2 * float(r.abs().max()),
                                       msg=lambda s: f"{name} {what}: {s}")


def test_resnet50_engages_its_sinks(cuda, monkeypatch, switch):
    """resnet50, batch 2, 64x64, one forward / backward from the same seed with the switch on and off: the fused GEMM
    serves the 5 identity blocks' bn3 of layers 1 and 2 and layer 1's stride-1 downsample BatchNorm -- 6 of the 13
    BatchNorms that only have dx to write behind a wide-K 1x1 convolution; the 7 identity blocks of layers 3 and 4
    (Cin 256 / 512: more than one N tile) stay on the two kernels, where the fused GEMM measured no faster
    (ops.conv1x1.dx_sink_for, profiles/bn_dx_fused.md).  With the deterministic weight
    gradients every BatchNorm-side gradient buffer of a wide-K 1x1 data gradient is bitwise equal between the two,
    and the flat gradients agree (cosine >= 0.999)."""
    from polyaxon_amd.models.resnet import resnet50
    from polyaxon_amd.ops import _native

    lib = _native.lib("plx_conv")
    lib.plx_set_tn_atomic(0)
    try:
        x = torch.randn(2, 3, 64, 64, device=cuda, generator=torch.Generator(device=cuda).manual_seed(3)).to(
            torch.bfloat16).contiguous(memory_format=torch.channels_last)
        tgt = torch.tensor([1, 7], device=cuda)
        flat, bufs, engaged = {}, {}, {}
        for on in (False, True):
            switch(on)
            torch.manual_seed(4)
            model = resnet50(num_classes=10, zero_init_residual=False).to(cuda).to(memory_format=torch.channels_last)
            log = []
            with monkeypatch.context() as mp:
                _spy(mp, log)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = F.cross_entropy(model(x).float(), tgt)
                del log[:]
                loss.backward()
            torch.cuda.synchronize()
            engaged[on] = sum(f for f, _ in log)
            bufs[on] = [a for _, a in log]                    # every 1x1 dgrad's gradient operand, in order
            flat[on] = torch.cat([p.grad.float().flatten() for p in model.parameters()])
        assert engaged == {False: 0, True: 6}, engaged
        assert len(bufs[True]) == len(bufs[False])
        for a, b in zip(bufs[True], bufs[False]):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), a.shape
        cos = float(F.cosine_similarity(flat[True], flat[False], dim=0))
        assert cos >= 0.999, cos
    finally:
        lib.plx_set_tn_atomic(int(os.environ.get("PLX_WGRAD_ATOMIC", "1")))


def test_replaced_gradient_raises(cuda, switch):
    """A hook that replaces the BatchNorm's (still unwritten) input gradient makes the convolution's backward raise
    instead of running on a tensor computed from uninitialised memory."""
    from polyaxon_amd.ops.conv1x1 import Conv1x1
    from polyaxon_amd.ops.norm import BatchNormAct

    conv, bn = Conv1x1(64, 128).to(cuda), BatchNormAct(128, act=True).to(cuda)
    x = torch.randn(2, 64, 4, 4, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    yc = conv(x)
    yc.register_hook(lambda grad: grad.clone())
    y = bn(yc)
    with pytest.raises(RuntimeError, match="DxSink"):
        y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
