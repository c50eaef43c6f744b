"""The BatchNorm-dx data gradient that also forms the convolution's weight gradient (csrc/conv_gemm.hip
plx_gemm_nt_bndx_wgrad, ops.conv1x1.gemm_nt_bndx_wgrad) vs plx_gemm_nt_bndx on the same inputs: dx and the
BatchNorm-backward partial rows bit for bit, dy never written, dW exact on integer data and within the fp32 summation
bound of its M terms on random data; and the two bottleneck kinds of ResNet layer 1 with the switch on and off."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N = 64
GUARD = 0x7B7B  # bf16 bit pattern of the dy sentinel and of the guard rows behind C
U = 2.0 ** -24  # unit roundoff of fp32
# (add, add_mask) x mask x bnr
OPTIONS = list(itertools.product(("none", "add", "add_mask"), (True, False), (True, False)))


def _pack_bits(keep: torch.Tensor) -> torch.Tensor:
    """bool [..] -> the 1-bit mask layout of bn_apply_kernel: bit k of byte i = element 8 i + k."""
    w = 2 ** torch.arange(8, device=keep.device, dtype=torch.int32)
    return (keep.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(m: int, k: int, integer: bool):
    """Inputs of one (M, K), computed once and shared read-only.  integer: g, x, x_in in [-4, 4] and integer
    coefficients with |dy| <= 3 * 4 + 3 * 4 + 8 = 32, so dy is exact in bf16 and every dW sum (< 1380 * 32 * 4 < 2^24)
    is exact in fp32 in any order."""
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(77 * m + k + int(integer))
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=dev, generator=gen).float()  # noqa: E731
    if integer:
        g, x, x_in = (ri(-4, 4, m, k).to(torch.bfloat16), ri(-4, 4, m, k).to(torch.bfloat16),
                      ri(-4, 4, m, N).to(torch.bfloat16))
        coef = torch.cat([ri(-3, 3, k), ri(-3, 3, k), ri(-8, 8, k)])
    else:
        g, x, x_in = rnd(m, k).to(torch.bfloat16), rnd(m, k).to(torch.bfloat16), rnd(m, N).to(torch.bfloat16)
        coef = torch.cat([torch.rand(k, device=dev, generator=gen) + 0.5, 0.3 * rnd(k), 0.1 * rnd(k)])
    keep = torch.rand(m, k, device=dev, generator=gen) > 0.4
    mask = _pack_bits(keep)                                   # K % 8 == 0: whole bytes
    wt = (rnd(N, k) / k ** 0.5).to(torch.bfloat16)
    add = rnd(m, N).to(torch.bfloat16)
    add_mask = _pack_bits(torch.rand(m, N, device=dev, generator=gen) > 0.5)
    xp = rnd(m, N).to(torch.bfloat16)                         # the BnBwd epilogue's operands
    keep_p = torch.rand(m, N, device=dev, generator=gen) > 0.3
    mean_p, invstd_p = 0.1 * rnd(N), torch.rand(N, device=dev, generator=gen) + 0.5
    torch.cuda.synchronize()
    return dict(g=g, x=x, x_in=x_in, coef=coef.contiguous(), keep=keep, mask=mask, wt=wt,
                add=add, add_mask=add_mask, xp=xp, keep_p=keep_p, mask_p=_pack_bits(keep_p), mean_p=mean_p,
                invstd_p=invstd_p)


def _run(case, m, k, opt, fused: bool, blocks: int = 0, dw=None):
    """One launch of plx_gemm_nt_bndx (fused=False) or plx_gemm_nt_bndx_wgrad; (dy buffer, C, partial rows)."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.conv1x1 import gemm_nt_bndx, gemm_nt_bndx_wgrad

    addk, use_mask, use_bnr = opt
    dev = case["g"].device
    dy = torch.full((m, k), GUARD, dtype=torch.int16, device=dev).view(torch.bfloat16)
    c_buf = torch.full((m + 8, N), GUARD, dtype=torch.int16, device=dev).view(torch.bfloat16)
    out = c_buf[:m]
    nblk = -(-m // 256)
    part = bnr = None
    if use_bnr:
        part = torch.full((2, nblk, N), float("nan"), device=dev)
        bnr = _native.GemmBnBwdArgs(case["xp"].data_ptr(), case["mask_p"].data_ptr(), case["mean_p"].data_ptr(),
                                    case["invstd_p"].data_ptr(), part.data_ptr(), nblk, 0)
    kw = dict(add=case["add"] if addk != "none" else None, bnr=bnr,
              add_mask=case["add_mask"] if addk == "add_mask" else None)
    mask = case["mask"] if use_mask else None
    if fused:
        gemm_nt_bndx_wgrad(case["g"], case["x"], mask, case["coef"], dy, case["wt"], case["x_in"], dw, out,
                           blocks=blocks, **kw)
    else:
        gemm_nt_bndx(case["g"], case["x"], mask, case["coef"], dy, case["wt"], out, **kw)
    torch.cuda.synchronize()
    assert (_bits(c_buf[m:]) == GUARD).all(), "rows of C past M were written"
    return dy, out, part


def _check_partials(case, m, opt, out, part):
    """part[0 | 1][t][n] vs fp64 sums of dz and dz * xhat over tile t's rows: 256 * 2^-24 * sum |term| per entry."""
    keep = case["keep_p"].double()
    dz = out.double() * keep
    xhat = (case["xp"].double() - case["mean_p"].double()) * case["invstd_p"].double()
    for which, term in ((0, dz), (1, dz * xhat)):
        for t in range(part.shape[1]):
            rows = term[t * 256:(t + 1) * 256]
            err = (part[which, t].double() - rows.sum(0)).abs()
            bound = 256 * U * rows.abs().sum(0)
            assert (err <= bound).all(), (which, t, float((err - bound).max()))


@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1380])
@pytest.mark.parametrize("k", [64, 256])
def test_kernel_random(cuda, k, m, blocks):
    """Every epilogue option on random data.  blocks = 2: M = 1380 makes each block walk three tiles, the last one
    ragged; M = 1 leaves one block without a tile.  dW starts from zero; the reference is the fp64 product of the
    bf16 dy that plx_gemm_nt_bndx stores with x_in, the bound gamma_M * sum |dy * x_in| that of any fp32 summation of
    the M exact bf16 x bf16 products per entry."""
    case = _case(m, k, False)
    gamma = m * U / (1 - m * U)
    for opt in OPTIONS:
        dy_ref, out_ref, part_ref = _run(case, m, k, opt, False)
        dw = torch.zeros(k, N, device=cuda)
        dy, out, part = _run(case, m, k, opt, True, blocks, dw)
        assert (_bits(dy) == GUARD).all(), f"{opt}: dy was written"
        assert torch.equal(_bits(out), _bits(out_ref)), f"{opt}: dx differs from plx_gemm_nt_bndx"
        if part is not None:
            assert torch.equal(part, part_ref), f"{opt}: partial rows differ from plx_gemm_nt_bndx"
            _check_partials(case, m, opt, out, part)
        ref = dy_ref.double().t() @ case["x_in"].double()
        bound = gamma * (dy_ref.double().abs().t() @ case["x_in"].double().abs())
        err = (dw.double() - ref).abs()
        print(f"{opt}: max |dW - ref| = {float(err.max()):.3g}, max of err / bound = "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3g}")
        assert (err <= bound).all(), f"{opt}: dW off by {float((err - bound).max()):.3g} beyond the bound"


@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1380])
@pytest.mark.parametrize("k", [64, 256])
def test_kernel_integer_exact(cuda, k, m, blocks):
    """Integer data (see _case): dW, pre-filled with integers, equals the int64 reference exactly, twice."""
    case = _case(m, k, True)
    a, b, d = case["coef"].view(3, k).long()
    pre = torch.randint(-50, 51, (k, N), device=cuda, generator=torch.Generator(device=cuda).manual_seed(m + k))
    for use_mask in (True, False):
        opt = ("add", use_mask, True)
        gm = case["g"].long() * (case["keep"].long() if use_mask else 1)
        dy_int = a * gm + b * case["x"].long() + d
        assert int(dy_int.abs().max()) <= 32
        dy_ref, _, _ = _run(case, m, k, opt, False)
        assert torch.equal(dy_ref.long(), dy_int), "plx_gemm_nt_bndx's dy is not the integer expression"
        # (integers below 2^53: the fp64 product is the int64 one, which the device has no matmul for)
        ref = pre + (dy_int.double().t() @ case["x_in"].double()).long()
        assert int(ref.abs().max()) < 2 ** 24
        got = []
        for _ in range(2):
            dw = pre.float()
            _run(case, m, k, opt, True, blocks, dw)
            got.append(dw)
            assert torch.equal(dw.long(), ref) and torch.equal(dw, dw.round()), float((dw.double() - ref).abs().max())
        assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("n,k", [(128, 256), (64, 320)])
def test_argument_checks(cuda, n, k):
    """N = 128 or K = 320: the error code, and nothing is launched (C, dW and dy keep their contents)."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.conv1x1 import _stream

    m = 64
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=cuda)  # noqa: E731
    g, x, wt, x_in = z(m, k), z(m, k), z(n, k), z(m, n)
    coef = torch.ones(3 * k, device=cuda)
    dy = torch.full((m, k), GUARD, dtype=torch.int16, device=cuda)
    out = torch.full((m, n), GUARD, dtype=torch.int16, device=cuda)
    dw = torch.full((k, n), 3.0, device=cuda)
    rc = _native.lib("plx_conv").plx_gemm_nt_bndx_wgrad(g.data_ptr(), x.data_ptr(), None, coef.data_ptr(),
                                                        dy.data_ptr(), wt.data_ptr(), out.data_ptr(), m, n, k, k, n,
                                                        None, 0, None, None, x_in.data_ptr(), dw.data_ptr(), n, 0,
                                                        _stream())
    torch.cuda.synchronize()
    assert rc == -1
    assert (dy == GUARD).all() and (out == GUARD).all() and (dw == 3.0).all()


@pytest.fixture
def switch():
    """ops.conv1x1.set_dgrad_wgrad_fused, restored afterwards."""
    from polyaxon_amd.ops import conv1x1

    prev = conv1x1.set_dgrad_wgrad_fused(True)
    yield conv1x1.set_dgrad_wgrad_fused
    conv1x1.set_dgrad_wgrad_fused(prev)


def _block(kind: str, cuda):
    from polyaxon_amd.models.resnet import Bottleneck, Downsample

    torch.manual_seed(21)
    if kind == "identity":
        blk, cin = Bottleneck(256, 64), 256
    else:
        blk, cin = Bottleneck(64, 64, 1, Downsample(64, 256, 1)), 64
    return blk.to(memory_format=torch.channels_last), cin


def _backward(blk, flat, x, g, monkeypatch, record):
    """One forward / backward of the block from zeroed flat gradients; (input gradient, {name: gradient}, fused calls).
    record: {weight slot address: (dy rows, x rows)} of every plx_gemm_tn weight gradient, filled when given."""
    from polyaxon_amd.ops import conv1x1

    calls = []
    with monkeypatch.context() as mp:
        real, real_tn = conv1x1.gemm_nt_bndx_wgrad, conv1x1.gemm_tn

        def counted(*a, **kw):
            calls.append(a[7].data_ptr())
            return real(*a, **kw)

        def tn(a, b, out=None, accumulate=False):
            if record is not None and out is not None:
                record[out.data_ptr()] = (a.detach().clone(), b.detach().clone())
            return real_tn(a, b, out=out, accumulate=accumulate)
        mp.setattr(conv1x1, "gemm_nt_bndx_wgrad", counted)
        mp.setattr(conv1x1, "gemm_tn", tn)
        flat.grads.zero_()
        xa = x.clone().requires_grad_()
        hook = None
        if record is not None:  # the 3x3 convolution's operands: its input, and the gradient of its output
            def grab(mod, inp, out):
                record["conv2"] = [inp[0].detach().clone()]
                out.register_hook(lambda gr: record["conv2"].append(gr.detach().clone()))
            hook = blk.conv2.register_forward_hook(grab)
        blk(xa).backward(g)
        if hook is not None:
            hook.remove()
    torch.cuda.synchronize()
    return xa.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()}, calls


@pytest.mark.parametrize("kind", ["identity", "downsample"])
def test_bottleneck_switch_on_off(cuda, monkeypatch, switch, kind):
    """Bottleneck(256, 64) (conv3 behind bn3's dx) and Bottleneck(64, 64, downsample) (the downsample conv behind its
    BatchNorm's dx) at batch 3, 10 x 10 (M = 300, two row tiles), gradients accumulated into flat slots.  On vs off: the
    input gradient and every BatchNorm gradient are bitwise equal (dx and the partial rows are), the fused path ran
    exactly once, for that convolution, and every convolution's weight gradient -- M terms per entry -- is within
    gamma_M * sum |dy * x| of the fp64 product of the bf16 operands the two-kernel path handed to its weight-gradient
    kernel (recorded in the off run; the on run's are bitwise the same), in both settings.  With the deterministic
    weight-gradient mode the fused path is not taken."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.flat import FlatParams

    blk, cin = _block(kind, cuda)
    flat = FlatParams(blk, cuda)
    flat.enable_direct_grads(True)
    blk.train()
    gen = torch.Generator(device=cuda).manual_seed(5)
    x = torch.randn(3, cin, 10, 10, device=cuda, generator=gen).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    g = torch.randn(3, 256, 10, 10, device=cuda, generator=gen).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    m = 300
    gamma = m * U / (1 - m * U)
    fused_w = blk.conv3.weight if kind == "identity" else blk.downsample.conv.weight
    fused_name = "conv3.weight" if kind == "identity" else "downsample.conv.weight"
    record = {}
    switch(False)
    dx_off, grads_off, calls = _backward(blk, flat, x, g, monkeypatch, record)
    assert calls == []
    switch(True)
    dx_on, grads_on, calls = _backward(blk, flat, x, g, monkeypatch, None)
    assert calls == [fused_w.grad.data_ptr()], calls
    assert torch.equal(_bits(dx_on), _bits(dx_off)), "input gradient differs on / off"
    slots = {p.grad.data_ptr(): n for n, p in blk.named_parameters()}
    x2, dy2 = record.pop("conv2")
    operands = {slots[ptr]: v for ptr, v in record.items()}
    assert fused_name in operands
    unf, dyf = F.unfold(x2.double(), 3, padding=1), dy2.double().flatten(2)    # [B][Cin * 9][L], [B][Cout][L]
    ref2 = torch.einsum("bol,bkl->ok", dyf, unf).view(64, 64, 3, 3)
    bound2 = gamma * torch.einsum("bol,bkl->ok", dyf.abs(), unf.abs()).view(64, 64, 3, 3)
    for name, off in grads_off.items():
        on = grads_on[name]
        if off.dim() == 1:
            assert torch.equal(on, off), f"{name} differs on / off"
        else:
            if name == "conv2.weight":
                ref, bound = ref2, bound2
            else:
                dy, xin = operands[name]
                ref = (dy.double().t() @ xin.double()).view(off.shape)
                bound = gamma * (dy.double().abs().t() @ xin.double().abs()).view(off.shape)
            for got, what in ((on, "on"), (off, "off")):
                err = (got.double() - ref).abs()
                print(f"{name} {what}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}")
                assert (err <= bound).all(), (name, what, float((err - bound).max()))
    lib = _native.lib("plx_conv")
    lib.plx_set_tn_atomic(0)
    try:
        _, _, calls = _backward(blk, flat, x, g, monkeypatch, None)
        assert calls == []
    finally:
        import os
        lib.plx_set_tn_atomic(int(os.environ.get("PLX_WGRAD_ATOMIC", "1")))
