"""A downsampling bottleneck's backward without the d_residual round trip (PLX_DS_BWD_FUSED, ops.conv1x1.ds_bwd_route):
bn3 returns its incoming gradient dy as the residual's gradient and the downsample BatchNorm masks it with bn3's ReLU
mask; on route A conv3's data gradient forms bn3's dx and the downsample BatchNorm runs its own reduce, on route B bn3's
dx pass stays (it still reduces that BatchNorm's partials) and only stops writing d_residual.

Every block is followed by an identity bottleneck, so bn3 gets its partials from a consumer's epilogue as in the model.
Switch 0 vs 1 (vs 2): what derives from bn3's dx -- the gradients reaching conv2 and conv1 and every BatchNorm
gradient of the main branch -- is bitwise equal on both routes; on route B, and above 2048 channels, so is everything
else (weight gradients compared in the deterministic weight-gradient mode: float atomics do not repeat bit for bit
from one run to the next).  Route A's downsample-BatchNorm sums run in another order (bn_bwd_reduce_kernel's partials,
not the dx pass's), so dgamma / dbeta are held to an fp64 oracle on the tensors the kernels read, with the bound of any
fp32 summation of the M terms (see :func:`_ds_oracle`), and the block-input gradient, whose chain (finalize, dx, a bf16
GEMM, the add of conv1's gradient) has no closed bound here, to at most twice switch 0's maximum error against an fp64
oracle of that chain on the same tensors (:func:`_x_oracle`).

Measured on an MI355X, max error / bound of the downsample BatchNorm, switch 0 | route A: case a dgamma 0.0029 | 0.0018,
case b dgamma 0.032 | 0.028; dbeta 0 | 0 in both (the sum of 300 or 50 bf16 terms is exact in fp32).  Block-input
gradient, max |error| against the oracle, switch 0 | route A: case a 0.0957 | 0.0957 (max |gradient| 18.8), case b
0.0394 | 0.0394 (max |gradient| 9.74).
"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
U = 2.0 ** -24  # unit roundoff of fp32

# name: (in, width, stride, N, H = W)
CASES = {"a": (64, 64, 1, 3, 10),      # layer-1 class: M = 300, ragged against the 256-row tile; route A + bndx_wgrad
         "b": (256, 128, 2, 2, 9),     # layer-2 class: odd side, uneven stride-2 parity classes; route B (1) or A (2)
         "c": (64, 1024, 1, 1, 4)}     # C = 4096: no ResBn above 2048 channels, d_residual stays


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def _pack_bits(keep: torch.Tensor) -> torch.Tensor:
    """bool [..] -> the 1-bit mask layout of bn_apply_kernel: bit k of byte i = element 8 i + k."""
    w = 2 ** torch.arange(8, device=keep.device, dtype=torch.int32)
    return (keep.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


@pytest.fixture
def knobs():
    """Sets (PLX_DS_BWD_FUSED mode, atomic weight gradients); restores both afterwards."""
    from polyaxon_amd.ops import _native, conv1x1

    lib = _native.lib("plx_conv")
    prev = conv1x1.set_ds_bwd_fused(1)

    def set_(mode: int, atomic: int = 1):
        conv1x1.set_ds_bwd_fused(mode)
        lib.plx_set_tn_atomic(atomic)
    yield set_
    conv1x1.set_ds_bwd_fused(prev)
    lib.plx_set_tn_atomic(int(os.environ.get("PLX_WGRAD_ATOMIC", "1")))


def _make(case: str, **kw):
    from polyaxon_amd.models.resnet import Bottleneck, Downsample

    cin, width, stride, _, _ = CASES[case]
    return torch.nn.Sequential(Bottleneck(cin, width, stride, Downsample(cin, 4 * width, stride, **kw), **kw),
                               Bottleneck(4 * width, width, **kw))


@functools.lru_cache(maxsize=None)
def _setup(case: str):
    """The two blocks (flat parameters, direct gradients), the input and the output's gradient: built once, read only."""
    from polyaxon_amd.ops.flat import FlatParams

    dev = torch.device("cuda", 0)
    cin, width, stride, n, side = CASES[case]
    torch.manual_seed(31)
    net = _make(case)
    with torch.no_grad():  # gammas and betas away from their initial 1 / 0
        for name, p in net.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.rand_like(p) + 0.5 if name.endswith("weight") else 0.2 * torch.randn_like(p))
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(memory_format=torch.channels_last)
    flat = FlatParams(net, dev)
    flat.enable_direct_grads(True)
    net.train()
    gen = torch.Generator(device=dev).manual_seed(9)
    so = (side - 1) // stride + 1
    x = torch.randn(n, cin, side, side, device=dev, generator=gen).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    g = torch.randn(n, 4 * width, so, so, device=dev, generator=gen).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    return net, flat, x, g, state


def _run(case: str):
    """One forward / backward from zeroed flat gradients under the current knobs.  Returns the gradients by name
    (parameters, "x", and the tensors reaching conv2 / conv1 of the first block), and what the downsample BatchNorm's
    backward saw: its input yd, its saved statistics, bn3's output and the gradients of both."""
    from polyaxon_amd.models.resnet import run_blocks

    net, flat, x, g, _ = _setup(case)
    blk = net[0]
    seen, hooks = {}, []

    def grab(key, inp=False):
        def fwd(mod, args, out):
            seen[key] = out
            out.register_hook(lambda gr: seen.__setitem__("d_" + key, gr))
            if inp:
                args[0].register_hook(lambda gr: seen.__setitem__("d_" + key + "_in", gr))
        return fwd
    for key, mod, inp in (("mid", blk, False), ("identity", blk.downsample, False), ("yd", blk.downsample.conv, False),
                          ("conv2", blk.conv2, True), ("conv1", blk.conv1, False)):
        hooks.append(mod.register_forward_hook(grab(key, inp)))
    flat.grads.zero_()
    xa = x.clone().requires_grad_()
    try:
        out = run_blocks(net, xa)
        link = seen["identity"]._plx_bn_link
        stats = (link.mean.detach().clone(), link.invstd.detach().clone())
        out.backward(g)
    finally:
        for h in hooks:
            h.remove()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in net.named_parameters()}
    grads.update(x=xa.grad.clone(), d_conv2=seen["d_conv2"].clone(), d_conv2_in=seen["d_conv2_in"].clone(),
                 d_conv1=seen["d_conv1"].clone())
    ctx = dict(yd=seen["yd"].detach(), mid=seen["mid"].detach(), g=seen["d_mid"], dres=seen["d_identity"], stats=stats)
    return grads, ctx


MAIN = ("0.conv1.", "0.bn1.", "0.conv2.", "0.bn2.", "0.conv3.", "0.bn3.", "1.")  # all but the downsample branch


def _same(a, b):
    return torch.equal(a, b) if a.dtype == torch.float32 else torch.equal(_bits(a), _bits(b))


def _assert_main_equal(on, off, weights: bool):
    """What derives from bn3's dx, bitwise: the tensors reaching conv2 and conv1, the main branch's (and the successor's)
    BatchNorm gradients, and with ``weights`` (deterministic mode) its weight gradients too."""
    for key in ("d_conv2", "d_conv2_in", "d_conv1"):
        assert _same(on[key], off[key]), key
    for name in off:
        if name.startswith(MAIN) and (off[name].dim() == 1 or weights):
            assert _same(on[name], off[name]), name


def _ds_oracle(ctx):
    """fp64 dbeta = sum dz and dgamma = sum dz * xhat of the downsample BatchNorm over its M rows per channel, from the
    tensors its backward reads: dz = g * [mid > 0] (bf16, exact), xhat = (yd - mean) * invstd with the saved fp32
    statistics.  Bounds: the kernels add M fp32 terms per channel in some order (row lanes, blocks, then fp64 over the
    partial rows) and round the result to fp32 once: (gamma_M + u) * sum |term|; a dgamma term is dz times
    fl(fl(yd - mean) * invstd), two roundings, and enters through one fmaf: another 3 u * sum |term|."""
    yd = ctx["yd"].permute(0, 2, 3, 1).reshape(-1, ctx["yd"].shape[1]).double()
    keep = (ctx["mid"].permute(0, 2, 3, 1).reshape(yd.shape) > 0).double()
    dz = ctx["g"].permute(0, 2, 3, 1).reshape(yd.shape).double() * keep
    mean, invstd = ctx["stats"][0].double(), ctx["stats"][1].double()
    t = dz * (yd - mean) * invstd
    m = yd.shape[0]
    gm = m * U / (1 - m * U)
    return (dz.sum(0), (gm + U) * dz.abs().sum(0)), (t.sum(0), (gm + 4 * U) * t.abs().sum(0))


def _ds_ratios(grads, ctx):
    (db, db_b), (dg, dg_b) = _ds_oracle(ctx)
    rg = float(((grads["0.downsample.bn.weight"].double() - dg).abs() / dg_b.clamp_min(1e-300)).max())
    rb = float(((grads["0.downsample.bn.bias"].double() - db).abs() / db_b.clamp_min(1e-300)).max())
    return rg, rb


def _x_oracle(case: str, ctx, d_conv1):
    """The block-input gradient in fp64 from the tensors the backward read: the downsample BatchNorm's dx (saved
    statistics, exact sums over dz = g * [mid > 0]) through the transposed downsample convolution, plus conv1's data
    gradient of the bf16 gradient that reached conv1 (bitwise the same with every setting), both with the weights
    rounded to bf16 as the GEMMs read them.  What the kernels add to it: the fp32 finalize, dx rounded to bf16, the GEMMs'
    fp32 sums and two bf16 roundings of the result -- no closed bound here, hence the comparison with switch 0."""
    blk, stride = _setup(case)[0][0], CASES[case][2]
    f = lambda t: t.detach().double().cpu().contiguous()  # noqa: E731
    yd, g = f(ctx["yd"]), f(ctx["g"])
    dz = g * (f(ctx["mid"]) > 0).double()
    per = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    mean, invstd, gamma = per(f(ctx["stats"][0])), per(f(ctx["stats"][1])), per(f(blk.downsample.bn.weight))
    m = yd.numel() / yd.shape[1]
    xhat = (yd - mean) * invstd
    dyd = gamma * invstd * (dz - dz.sum((0, 2, 3), keepdim=True) / m
                            - xhat * (dz * xhat).sum((0, 2, 3), keepdim=True) / m)
    wd, w1 = f(blk.downsample.conv.weight.detach().bfloat16()), f(blk.conv1.weight.detach().bfloat16())
    x0 = torch.zeros(_setup(case)[2].shape, dtype=torch.float64, requires_grad=True)
    ((F.conv2d(x0, wd, stride=stride) * dyd).sum() + (F.conv2d(x0, w1) * f(d_conv1)).sum()).backward()
    return x0.grad


def _x_errors(case: str, off, ctx_off, on, ctx):
    """max |block-input gradient - oracle| with switch 0 and with the setting under test, printed."""
    e_off = float((off["x"].double().cpu() - _x_oracle(case, ctx_off, off["d_conv1"])).abs().max())
    ref = _x_oracle(case, ctx, on["d_conv1"])
    e_on = float((on["x"].double().cpu() - ref).abs().max())
    print(f"case {case} block-input gradient, max |error| vs fp64: switch 0 {e_off:.4g}, route A {e_on:.4g}"
          f" (max |gradient| {float(ref.abs().max()):.4g})")
    return e_off, e_on


def _fused_calls(monkeypatch, case):
    """Runs the case once; the weight slots plx_gemm_nt_bndx_wgrad was called for."""
    from polyaxon_amd.ops import conv1x1

    calls = []
    with monkeypatch.context() as mp:
        real = conv1x1.gemm_nt_bndx_wgrad
        mp.setattr(conv1x1, "gemm_nt_bndx_wgrad", lambda *a, **kw: (calls.append(a[7].data_ptr()), real(*a, **kw))[1])
        out = _run(case)
    return out, calls


@gpu
def test_route_a_layer1(cuda, knobs, monkeypatch):
    """Case a, switch 1 = route A: conv3 and the downsample conv both form their weight gradient inside the BatchNorm-dx
    data gradient (no dx3, no d_residual: the residual's gradient is bn3's dy itself)."""
    net = _setup("a")[0]
    # the successor's conv3 (an identity block's) and the downsample conv take the fused kernel with either setting
    before = [net[1].conv3.weight.grad.data_ptr(), net[0].downsample.conv.weight.grad.data_ptr()]
    knobs(0)
    (off, ctx_off), calls = _fused_calls(monkeypatch, "a")
    assert sorted(calls) == sorted(before)
    assert ctx_off["dres"].data_ptr() != ctx_off["g"].data_ptr()
    knobs(1)
    (on, ctx), calls = _fused_calls(monkeypatch, "a")
    assert sorted(calls) == sorted(before + [net[0].conv3.weight.grad.data_ptr()])
    assert ctx["dres"].data_ptr() == ctx["g"].data_ptr(), "the residual's gradient is not bn3's dy itself"
    _assert_main_equal(on, off, weights=False)
    for what, (grads, c) in (("switch 0", (off, ctx_off)), ("route A", (on, ctx))):
        rg, rb = _ds_ratios(grads, c)
        print(f"case a {what}: downsample BatchNorm dgamma {rg:.3g} dbeta {rb:.3g} (max error / bound)")
        assert rg <= 1.0 and rb <= 1.0, (what, rg, rb)
    e_off, e_on = _x_errors("a", off, ctx_off, on, ctx)
    assert e_on <= 2.0 * e_off


@gpu
def test_route_b_layer1_deterministic(cuda, knobs, monkeypatch):
    """Case a with the deterministic weight-gradient mode: no fused weight gradient, so route B -- every gradient bitwise
    equal to switch 0's, and no d_residual."""
    knobs(0, atomic=0)
    off, _ = _run("a")
    knobs(1, atomic=0)
    (on, ctx), calls = _fused_calls(monkeypatch, "a")
    assert calls == []
    assert ctx["dres"].data_ptr() == ctx["g"].data_ptr()
    for name in off:
        assert _same(on[name], off[name]), name


@gpu
@pytest.mark.parametrize("mode", [1, 2], ids=["route_b", "route_a"])
def test_layer2_routes(cuda, knobs, mode):
    """Case b (strided block) on each route, deterministic weight gradients.  Route B: everything bitwise equal to
    switch 0.  Route A (mode 2): the main branch bitwise, the downsample BatchNorm within the oracle's bound, the block
    input gradient within twice switch 0's error."""
    knobs(0, atomic=0)
    off, ctx_off = _run("b")
    knobs(mode, atomic=0)
    on, ctx = _run("b")
    assert ctx["dres"].data_ptr() == ctx["g"].data_ptr() != ctx_off["dres"].data_ptr()
    _assert_main_equal(on, off, weights=True)
    for what, (grads, c) in (("switch 0", (off, ctx_off)), (f"switch {mode}", (on, ctx))):
        rg, rb = _ds_ratios(grads, c)
        print(f"case b {what}: downsample BatchNorm dgamma {rg:.3g} dbeta {rb:.3g} (max error / bound)")
        assert rg <= 1.0 and rb <= 1.0, (what, rg, rb)
    if mode == 1:
        for name in off:
            assert _same(on[name], off[name]), name
        return
    e_off, e_on = _x_errors("b", off, ctx_off, on, ctx)
    assert e_on <= 2.0 * e_off


@gpu
def test_above_2048_channels_falls_back(cuda, knobs):
    """Case c (C = 4096): the dx pass takes no ResBn there, d_residual is still written, and every gradient is bitwise
    switch 0's."""
    knobs(0, atomic=0)
    off, _ = _run("c")
    knobs(1, atomic=0)
    on, ctx = _run("c")
    assert ctx["dres"].data_ptr() != ctx["g"].data_ptr()
    for name in off:
        assert _same(on[name], off[name]), name


@gpu
def test_no_dres_allocation(cuda, knobs):
    """Switch 1 makes exactly one allocation fewer in a forward + backward than switch 0, d_residual's (route B), and
    the residual's gradient is bn3's dy itself."""
    _, _, x, g, _ = _setup("b")
    act = g.numel() * 2
    peaks = {}
    for mode in (0, 1):
        knobs(mode, atomic=0)
        _run("b")  # warm: caches and workspaces exist
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        _, ctx = _run("b")
        peaks[mode] = (torch.cuda.memory_stats()["allocation.all.allocated"] - before, ctx)
    assert peaks[1][0] == peaks[0][0] - 1, "exactly one allocation fewer: d_residual"
    assert peaks[1][1]["dres"].data_ptr() == peaks[1][1]["g"].data_ptr() and peaks[1][1]["dres"].numel() * 2 == act


@functools.lru_cache(maxsize=None)
def _integer_case():
    """M = 512 rows (two row tiles), K = 256 channels behind a 64-channel input: small integers everywhere, statistics
    with invstd = 1 and integer means, and partial rows for bn3 that make its k2 = a, k3 = b integers per channel.  Then
    bn3's dx = A dz + B y3 + D is an integer of magnitude <= 2 * 4 + 2 * 4 + 2 + 4 = 22 (exact in bf16), every dW sum
    stays below 512 * 22 * 4 < 2^24, and the downsample BatchNorm's sums of dz and dz * xhat (|xhat| <= 6) below
    512 * 4 * 6 < 2^24: all exact in fp32 in any order."""
    dev = torch.device("cuda", 0)
    m, k, n = 512, 256, 64
    gen = torch.Generator(device=dev).manual_seed(123)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=dev, generator=gen).float()  # noqa: E731
    bf = torch.bfloat16
    g, y3, yd, x_in = ri(-4, 4, m, k).to(bf), ri(-4, 4, m, k).to(bf), ri(-4, 4, m, k).to(bf), ri(-4, 4, m, n).to(bf)
    keep = torch.rand(m, k, device=dev, generator=gen) > 0.4
    sign = lambda *s: ri(0, 1, *s) * 2 - 1  # noqa: E731
    gamma3, gammad = sign(k) * ri(1, 2, k), sign(k) * ri(1, 2, k)
    mean3, meand = ri(-2, 2, k), ri(-2, 2, k)
    one = torch.ones(k, device=dev)
    a, b = ri(-1, 1, k), ri(-1, 1, k)
    part = torch.zeros(2, 2, k, device=dev)  # two partial rows: sum dz = M a, sum dz xhat = M b, split unevenly
    part[0, 0], part[0, 1], part[1, 0], part[1, 1] = 3 * m * a, -2 * m * a, -m * b, 2 * m * b
    wt = ri(-2, 2, n, k).to(bf)
    torch.cuda.synchronize()
    return dict(m=m, k=k, n=n, g=g, y3=y3, yd=yd, x_in=x_in, keep=keep, mask=_pack_bits(keep), gamma3=gamma3,
                gammad=gammad, mean3=mean3, meand=meand, one=one, part=part.contiguous(), wt=wt)


def _integer_chain(c, fused: bool):
    """The native calls of layer 1.0's backward from bn3 to the block input's downsample part: switch 0's (dx pass with
    d_residual and ResBn, downsample BatchNorm from those, plx_gemm_nt + plx_gemm_tn for conv3) or route A's."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import _counters, _workspace, bn_backward
    from polyaxon_amd.ops.conv1x1 import gemm_nt, gemm_nt_bndx_wgrad, gemm_tn

    dev = c["g"].device
    m, k, n = c["m"], c["k"], c["n"]
    f32 = dict(dtype=torch.float32, device=dev)
    o = dict(dg3=torch.zeros(k, **f32), db3=torch.zeros(k, **f32), dgd=torch.zeros(k, **f32), dbd=torch.zeros(k, **f32),
             dxd=torch.empty(m, k, dtype=torch.bfloat16, device=dev), dw=torch.zeros(k, n, **f32),
             dx=torch.empty(m, n, dtype=torch.bfloat16, device=dev))
    coef3, coefd = torch.empty(3 * k, **f32), torch.empty(3 * k, **f32)
    dx3 = torch.empty(m, k, dtype=torch.bfloat16, device=dev)
    bn3 = dict(x=c["y3"], mask=c["mask"], dy=c["g"], m=m, c=k, gamma=c["gamma3"], save_mean=c["mean3"],
               save_invstd=c["one"], dgamma=o["dg3"], dbeta=o["db3"], coef=coef3, ext_part=c["part"], ext_nblk=2,
               workspace=_workspace(m, k, c["part"], 2, dev), relu=True, counters=_counters(dev))
    bnd = dict(x=c["yd"], m=m, c=k, gamma=c["gammad"], save_mean=c["meand"], save_invstd=c["one"], dgamma=o["dgd"],
               dbeta=o["dbd"], coef=coefd, dx=o["dxd"], counters=_counters(dev))
    if fused:
        bn_backward(**bn3)  # reduce / finalize only
        gemm_nt_bndx_wgrad(c["g"], c["y3"], c["mask"], coef3, dx3, c["wt"], c["x_in"], o["dw"], o["dx"])
        bn_backward(dy=c["g"], mask=c["mask"], relu=True, workspace=_workspace(m, k, None, 0, dev), **bnd)
    else:
        dres = torch.empty(m, k, dtype=torch.bfloat16, device=dev)
        nb = _native.size("plx_bn", "plx_bn_dx_blocks", m, k)
        rpart = torch.empty(2 * nb * k, **f32)
        rb = _native.ResBnArgs(c["yd"].data_ptr(), None, c["meand"].data_ptr(), c["one"].data_ptr(), rpart.data_ptr())
        bn_backward(dx=dx3, dres=dres, resbn=rb, **bn3)
        bn_backward(dy=dres, ext_part=rpart, ext_nblk=nb, workspace=_workspace(m, k, rpart, nb, dev), **bnd)
        gemm_nt(dx3, c["wt"], o["dx"])
        gemm_tn(dx3, c["x_in"], out=o["dw"], accumulate=True)
    torch.cuda.synchronize()
    return o


@gpu
def test_integer_data_exact(cuda, knobs):
    """Exactly representable data (:func:`_integer_case`): route A's calls give every gradient exactly as switch 0's,
    dW from float atomics included, and dW / the downsample BatchNorm's sums equal the integer reference."""
    knobs(1, atomic=1)
    c = _integer_case()
    off, on = _integer_chain(c, False), _integer_chain(c, True)
    for name in off:
        assert _same(on[name], off[name]), name
    dz = c["g"].double() * c["keep"].double()
    a, b = c["part"][0].sum(0).double() / c["m"], c["part"][1].sum(0).double() / c["m"]
    g3, mu3 = c["gamma3"].double(), c["mean3"].double()
    dx3 = g3 * (dz - a - (c["y3"].double() - mu3) * b)
    assert float(dx3.abs().max()) <= 22
    assert torch.equal(on["dw"].double(), dx3.t() @ c["x_in"].double())
    assert torch.equal(on["dbd"].double(), dz.sum(0))
    assert torch.equal(on["dgd"].double(), (dz * (c["yd"].double() - c["meand"].double())).sum(0))


@gpu
def test_refused_calls_launch_nothing(cuda):
    """A ResBn with neither dres nor dx, relu = 1 without a mask (own or foreign), and every mismatch between no_dres
    and what is passed are refused before any launch: every output keeps its sentinel."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import bn_backward

    lib = _native.lib("plx_bn")
    torch.manual_seed(4)
    m, c = 18, 64
    sentinel = {torch.bfloat16: -7.0, torch.float32: -12345.0, torch.int32: 77}
    outs = {}

    def out(name, numel, dtype=torch.float32):
        outs[name] = torch.full((numel,), sentinel[dtype], dtype=dtype, device=cuda)
        return outs[name]

    f32 = dict(dtype=torch.float32, device=cuda)
    x = torch.randn(m, c, device=cuda).to(torch.bfloat16)
    dy, x2 = torch.randn_like(x), torch.randn_like(x)
    gamma, mean, inv = torch.rand(c, **f32) + 0.5, torch.randn(c, **f32), torch.rand(c, **f32) + 0.5
    mask = torch.randint(0, 256, (m * c // 8,), device=cuda, dtype=torch.int32).to(torch.uint8)
    rpart = out("resbn_part", 2 * int(lib.plx_bn_dx_blocks(m, c)) * c)
    resbn = _native.ResBnArgs(x2.data_ptr(), None, mean.data_ptr(), inv.data_ptr(), rpart.data_ptr())
    bwd = dict(x=x, dy=dy, m=m, c=c, gamma=gamma, save_mean=mean, save_invstd=inv, dgamma=out("dgamma", c),
               dbeta=out("dbeta", c), coef=out("coef", 3 * c), workspace=out("workspace", int(lib.plx_bn_workspace(m, c))),
               relu=True, counters=out("counters", 64, torch.int32))
    dx, dres = out("dx", m * c, torch.bfloat16), out("dres", m * c, torch.bfloat16)
    for kw in (dict(bwd, mask=mask, dx=None, dres=None, resbn=resbn, no_dres=True),  # no pass for the ResBn to run in
               dict(bwd, mask=None, dx=dx),                            # relu = 1 (a foreign mask's case too), no mask
               dict(bwd, mask=mask, dx=dx, resbn=resbn),               # a ResBn without dres, not declared (no_dres)
               dict(bwd, mask=mask, dx=dx, dres=dres, resbn=resbn, no_dres=True),  # declared, yet dres is passed
               dict(bwd, mask=mask, dx=dx, no_dres=True)):             # declared without a ResBn
        with pytest.raises(RuntimeError, match="failed with code"):
            bn_backward(**kw)
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == sentinel[t.dtype]).all()), f"{name} was written by a refused call"


@gpu
def test_resbn_without_dres_matches_with(cuda):
    """The dx pass with a ResBn and dres = nullptr (the DRES = false instantiations) writes dx and the ResBn partial
    rows bit for bit as the pass that also stores d_residual; ragged M, one and several blocks."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import _counters, _workspace, bn_backward

    lib = _native.lib("plx_bn")
    gen = torch.Generator(device=cuda).manual_seed(8)
    for m, c in ((300, 256), (50, 512), (4099, 64)):
        f32 = dict(dtype=torch.float32, device=cuda)
        rnd = lambda *s: torch.randn(*s, device=cuda, generator=gen)  # noqa: E731
        x, dy, x2 = rnd(m, c).to(torch.bfloat16), rnd(m, c).to(torch.bfloat16), rnd(m, c).to(torch.bfloat16)
        mask = _pack_bits(torch.rand(m, c, device=cuda, generator=gen) > 0.4)
        gamma, mean, inv = torch.rand(c, **f32) + 0.5, rnd(c), torch.rand(c, **f32) + 0.5
        nb = int(lib.plx_bn_dx_blocks(m, c))
        res = []
        for with_dres in (True, False):
            dx = torch.full((m + 4, c), -7.0, dtype=torch.bfloat16, device=cuda)
            dres = torch.full((m + 4, c), -7.0, dtype=torch.bfloat16, device=cuda)
            rpart = torch.full((2 * nb * c,), float("nan"), **f32)
            rb = _native.ResBnArgs(x2.data_ptr(), None, mean.data_ptr(), inv.data_ptr(), rpart.data_ptr())
            dgb, coef = torch.empty(2 * c, **f32), torch.empty(3 * c, **f32)
            bn_backward(x=x, mask=mask, dy=dy, dx=dx, dres=dres if with_dres else None, m=m, c=c, gamma=gamma,
                        save_mean=mean, save_invstd=inv, dgamma=dgb, dbeta=dgb[c:], coef=coef,
                        workspace=_workspace(m, c, None, 0, cuda), relu=True, resbn=rb, counters=_counters(cuda),
                        no_dres=not with_dres)
            torch.cuda.synchronize()
            assert bool((dx[m:] == -7.0).all()) and bool((dres[m:] == -7.0).all()), "rows past M were written"
            assert with_dres or bool((dres == -7.0).all()), "dres was written without being passed"
            res.append((dx, rpart, dgb, coef))
        for got, want in zip(res[1], res[0]):
            assert _same(got, want)


def test_routing_rules():
    """ds_bwd_route on the channel counts of ResNet-50's four downsampling blocks (no GPU: the weight-gradient mode is
    passed in).  Layer 1 class: A, but B with the deterministic weight gradients; layer 2 class: B, A with mode 2; layers
    3 and 4: B whatever the mode (conv3 has no dx sink); above 2048 channels and with mode 0: off."""
    from polyaxon_amd.ops.conv1x1 import ds_bwd_route, dx_sink_shape_ok

    def route(cin, cout, mode, atomic=True):
        fused = atomic and cin == 64 and cout <= 256  # dgrad_wgrad_fused_ok's shape class, atomic mode
        return ds_bwd_route(cin, cout, dx_sink_shape_ok(cin, cout), mode=mode, wgrad_fused=fused)

    assert [route(64, 256, md) for md in (0, 1, 2)] == ["off", "A", "A"]
    assert [route(64, 256, md, atomic=False) for md in (0, 1, 2)] == ["off", "B", "A"]
    assert [route(128, 512, md) for md in (0, 1, 2)] == ["off", "B", "A"]
    for cin, cout in ((256, 1024), (512, 2048)):
        assert [route(cin, cout, md) for md in (0, 1, 2)] == ["off", "B", "B"]
    assert [route(1024, 4096, md) for md in (0, 1, 2)] == ["off", "off", "off"]
    assert [route(64, 4096, md) for md in (0, 1, 2)] == ["off", "off", "off"]
    # bn3 still runs a reduce of its own (no consumer served its partials): the dx pass stays
    assert ds_bwd_route(64, 256, False, mode=1, wgrad_fused=True) == "B"
