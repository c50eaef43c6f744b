"""The single-workgroup BatchNorm reduce + finalize (``PLX_BN_FIN_SINGLE=1``, csrc/bn_kernels.hip
``bn_*_finalize_single_kernel``) against the two paths it must agree with bit for bit (``torch.equal``), in one process
through ``plx_bn_set_fin_single``, on identical partials:

* the ticket kernels (switch off), whose parameter loads this change moved ahead of the row loads, and
* the reduce kernel followed by the finalize kernel (``counters = None``), which this change does not touch.

T = 512 partial rows is the largest count the single-workgroup kernels take.  Row counts: 1 and 2 (a single lane
group), 63 / 64 / 65 (a ragged split, a full one, a second split of one row), 98 and 392 (ResNet-50's 7x7 and 14x14
stages: the two-split and the eight-split instantiation), 511 / 512 (the last ragged and the last full split of the
single path) and 513 (the first count back on the ticket path).  C = 8 leaves most of a workgroup's channels past
the end, 64 is one workgroup, 128 two, 1024 and 2048 the wide layers.  Every output lives between sentinel margins that
must stay intact; on the single path the level-2 rows and the counters must not be written at all.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 512
PAD = 64
SENTINEL = -12345.0
NBLKS = [1, 2, 63, 64, 65, 98, 392, T - 1, T, T + 1]
CS = [8, 64, 128, 1024, 2048]
SINGLE, TICKET = 2, 1


class Guarded:
    """A float32 tensor of ``numel`` elements with PAD sentinel elements before and after it."""

    def __init__(self, numel, dev, fill=None):
        self.all = torch.full((numel + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.all[PAD:PAD + numel]
        if fill is not None:
            self.t.copy_(fill)

    def check(self):
        s = torch.full((PAD,), SENTINEL, dtype=torch.float32, device=self.all.device)
        assert torch.equal(self.all[:PAD], s) and torch.equal(self.all[-PAD:], s), "a kernel wrote outside its output"
        return self.t

    def untouched(self):
        return bool((self.all == SENTINEL).all())


def _lib():
    from polyaxon_amd.ops import _native

    return _native.lib("plx_bn")


@pytest.fixture(autouse=True)
def _restore_switch():
    yield
    _lib().plx_bn_set_fin_single(1)


_PART = {}


def _partials(nblk, c, dev):
    """Level-1 partials [2][nblk][C], made once per shape and never written: a signed sum and a positive one."""
    if (nblk, c) not in _PART:
        gen = torch.Generator(device="cpu").manual_seed(5000 + 17 * nblk + c)
        a = torch.randn(nblk, c, generator=gen) * 3.0
        b = torch.rand(nblk, c, generator=gen) * 9.0 + 1.0
        gamma = torch.rand(c, generator=gen) + 0.5
        beta = torch.randn(c, generator=gen) * 0.3
        mean = torch.randn(c, generator=gen) * 0.2
        invstd = torch.rand(c, generator=gen) + 0.5
        old = torch.randn(4, c, generator=gen)  # running_mean, running_var | dgamma, dbeta before the call
        _PART[(nblk, c)] = tuple(t.to(dev).contiguous() for t in (torch.stack([a, b]), gamma, beta, mean, invstd, old))
    return _PART[(nblk, c)]


# mode: 1 = switch on, 0 = switch off, None = no counters (reduce + finalize kernels back to back)
def _counters(mode, cnt):
    _lib().plx_bn_set_fin_single(1 if mode is None else mode)
    return None if mode is None else cnt


def _forward(mode, nblk, c, dev, cnt, running, part=None, x=None, m=None):
    from polyaxon_amd.ops.bn_fused import bn_forward

    lib = _lib()
    p, gamma, beta, _, _, old = _partials(nblk, c, dev)
    if part is not None:
        p = part
    m = nblk * 7 if m is None else m
    stats = Guarded(4 * c, dev)  # mean | invstd | scale | bias
    run = Guarded(2 * c, dev, fill=old[:2].reshape(-1))
    own = x is not None
    nws = int(lib.plx_bn_workspace(m, c)) if own else int(lib.plx_bn_l2_workspace(nblk, c))
    ws = Guarded(nws, dev)
    bn_forward(x=x, m=m, c=c, gamma=gamma, beta=beta, eps=1e-5, momentum=0.1, save_mean=stats.t,
               save_invstd=stats.t[c:], scale_bias=stats.t[2 * c:], workspace=ws.t,
               running_mean=run.t if running else None, running_var=run.t[c:] if running else None,
               ext_part=None if own else p, ext_nblk=0 if own else nblk, counters=_counters(mode, cnt))
    torch.cuda.synchronize()
    ws.check()
    return (stats.check().clone(), run.check().clone()), ws


def _backward(mode, nblk, c, dev, cnt, accumulate, part=None):
    from polyaxon_amd.ops.bn_fused import bn_backward

    lib = _lib()
    p, gamma, _, mean, invstd, old = _partials(nblk, c, dev)
    if part is not None:
        p = part
    dgb = Guarded(2 * c, dev, fill=old[2:].reshape(-1))
    coef = Guarded(3 * c, dev)
    ws = Guarded(int(lib.plx_bn_l2_workspace(nblk, c)), dev)
    bn_backward(x=None, dy=None, m=nblk * 7, c=c, gamma=gamma, save_mean=mean, save_invstd=invstd, dgamma=dgb.t,
                dbeta=dgb.t[c:], coef=coef.t, workspace=ws.t, ext_part=p, ext_nblk=nblk, accumulate=accumulate,
                counters=_counters(mode, cnt))
    torch.cuda.synchronize()
    ws.check()
    return (dgb.check().clone(), coef.check().clone()), ws


def _same(outs):
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    assert all(bool(torch.isfinite(t).all()) for t in outs[0])


def _check_path(lib, nblk, c, cnt, ws_on):
    """What the switch-on call ran: the rule, and on the single path neither level-2 rows nor counters written."""
    single = nblk <= T
    assert lib.plx_bn_fin_path(nblk, c) == (SINGLE if single else TICKET)
    assert ws_on.untouched() == single
    assert int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("nblk", NBLKS)
def test_forward_bit_identical(cuda, nblk, c):
    lib = _lib()
    cnt = torch.zeros(64, dtype=torch.int32, device=cuda)
    for running in (True, False):
        runs = [_forward(mode, nblk, c, cuda, cnt, running) for mode in (1, 0, None, 1)]
        _same([r[0] for r in runs])
        lib.plx_bn_set_fin_single(1)
        _check_path(lib, nblk, c, cnt, runs[0][1])
        if not running:  # the running statistics were left alone
            assert torch.equal(runs[0][0][1], _partials(nblk, c, cuda)[5][:2].reshape(-1))


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("nblk", NBLKS)
def test_backward_bit_identical(cuda, nblk, c):
    lib = _lib()
    cnt = torch.zeros(64, dtype=torch.int32, device=cuda)
    for accumulate in (0, 1):
        runs = [_backward(mode, nblk, c, cuda, cnt, accumulate) for mode in (1, 0, None, 1)]
        _same([r[0] for r in runs])
        lib.plx_bn_set_fin_single(1)
        _check_path(lib, nblk, c, cnt, runs[0][1])


def test_counters_stay_zero_for_the_ticket_path(cuda):
    """Single-path calls leave the shared counter array zeroed, so a ticket-path call right behind them on the same
    array (nblk = T + 1: nine workgroups per channel group draw tickets) still finds its last arriver."""
    c = 128
    cnt = torch.zeros(64, dtype=torch.int32, device=cuda)
    for nblk in (98, 392, T):
        _forward(1, nblk, c, cuda, cnt, True)
        _backward(1, nblk, c, cuda, cnt, 1)
    assert int(cnt.abs().sum()) == 0
    fwd = [_forward(mode, T + 1, c, cuda, cnt, True)[0] for mode in (1, None)]
    bwd = [_backward(mode, T + 1, c, cuda, cnt, 1)[0] for mode in (1, None)]
    _same(fwd)
    _same(bwd)
    assert int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("nblk", [98, 392, T + 1])
def test_integer_partials_sum_exactly(cuda, nblk):
    """Small-integer partials: every partial sum is an integer below 2^24, so dbeta and dgamma are the exact column
    sums on every path, whatever the order of the additions."""
    c = 64
    gen = torch.Generator(device="cpu").manual_seed(31 + nblk)
    part = torch.randint(-8, 9, (2, nblk, c), generator=gen).float().to(cuda)
    want = part.double().sum(1).float()  # [dbeta | dgamma]
    cnt = torch.zeros(64, dtype=torch.int32, device=cuda)
    for mode in (1, 0, None):
        (dgb, _), _ = _backward(mode, nblk, c, cuda, cnt, 0, part=part)
        assert torch.equal(dgb[c:], want[0]) and torch.equal(dgb[:c], want[1])


def test_own_statistics_pass(cuda):
    """A forward that runs its own statistics pass: the finalize adds row 0 of x, the shift of that pass, back."""
    lib = _lib()
    m, c = 3000, 64
    n = int(lib.plx_bn_workspace(m, c)) // (2 * c)  # nblk + ceil(nblk / 64)
    nblk = next(b for b in range(1, n + 1) if b + (b + 63) // 64 == n)
    assert lib.plx_bn_fin_path(nblk, c) == SINGLE
    gen = torch.Generator(device="cpu").manual_seed(77)
    x = (torch.randn(m, c, generator=gen) * 2.0 + 5.0).to(torch.bfloat16).to(cuda)
    cnt = torch.zeros(64, dtype=torch.int32, device=cuda)
    runs = [_forward(mode, nblk, c, cuda, cnt, True, x=x, m=m) for mode in (1, 0, None)]
    _same([r[0] for r in runs])
    # on the single path the level-2 rows behind the level-1 partials stay unwritten
    assert bool((runs[0][1].t[2 * nblk * c:] == SENTINEL).all())
    mean = runs[0][0][0][:c]
    assert torch.allclose(mean, x.float().mean(0), atol=2e-2)  # the shift came back: the mean is near 5, not near 0


def test_stem_backward(cuda):
    """The stem's BatchNorm + pool backward at N = 2, 16 x 16, C = 64: its reduce + finalize takes the same switch."""
    lib = _lib()
    n, h, w, c = 2, 16, 16, 64
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    f32 = dict(dtype=torch.float32, device=cuda)
    gen = torch.Generator(device="cpu").manual_seed(4)
    x = torch.randn(n, h, w, c, generator=gen).to(torch.bfloat16).to(cuda)
    dy = torch.randn(n, oh, ow, c, generator=gen).to(torch.bfloat16).to(cuda)
    gamma, beta = (torch.rand(c, generator=gen) + 0.5).to(cuda), (torch.randn(c, generator=gen) * 0.3).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    cnt = torch.zeros(64, dtype=torch.int32, device=cuda)
    y = torch.empty(n, oh, ow, c, dtype=torch.bfloat16, device=cuda)
    idx = torch.empty(n * oh * ow * c, dtype=torch.uint8, device=cuda)
    stats = torch.empty(4 * c, **f32)
    fws = torch.empty(int(lib.plx_bn_workspace(n * h * w, c)), **f32)
    rm, rv = torch.zeros(c, **f32), torch.ones(c, **f32)
    rc = lib.plx_stem_bn_pool_forward(x.data_ptr(), y.data_ptr(), idx.data_ptr(), n, h, w, c, gamma.data_ptr(),
                                      beta.data_ptr(), 1e-5, 0.1, rm.data_ptr(), rv.data_ptr(), stats.data_ptr(),
                                      stats[c:].data_ptr(), stats[2 * c:].data_ptr(), fws.data_ptr(), None, 0,
                                      cnt.data_ptr(), st)
    assert rc == 0
    outs = []
    for mode in (1, 0, None):
        dx = Guarded(n * h * w * c // 2, cuda)  # bf16 elements, two to a float
        dgb = Guarded(2 * c, cuda, fill=torch.ones(2 * c, **f32))
        coef = Guarded(3 * c, cuda)
        ws = Guarded(int(lib.plx_stem_bn_pool_bwd_workspace(n, h, w, c)), cuda)
        cp = _counters(mode, cnt)
        rc = lib.plx_stem_bn_pool_backward(dy.data_ptr(), idx.data_ptr(), x.data_ptr(), dx.t.data_ptr(), n, h, w, c,
                                           gamma.data_ptr(), stats.data_ptr(), stats[c:].data_ptr(),
                                           stats[2 * c:].data_ptr(), dgb.t.data_ptr(), dgb.t[c:].data_ptr(),
                                           coef.t.data_ptr(), ws.t.data_ptr(), 1, None if cp is None else cp.data_ptr(),
                                           st)
        assert rc == 0
        torch.cuda.synchronize()
        ws.check()
        outs.append((dx.check().clone(), dgb.check().clone(), coef.check().clone()))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert int(cnt.abs().sum()) == 0
