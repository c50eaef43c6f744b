"""Residual dropout inside the fused add + norm kernels (csrc/rmsnorm.hip ``plx_add_ln_drop_*``,
``plx_add_rms_drop_*``) and its standalone pass ``plx_dropout``, on the GPU against the contract of ops/dropout.py:

* the kept set is ``mask_reference`` bit for bit, in the forward and in the backward;
* ``s`` within one bf16 rounding (plus fp32 slack) of the fp64 ``x + m c res``; ``y`` / ``mean`` / ``rstd`` bitwise
  those of the plain norm applied to ``s``;
* ``dx`` and the ``dw`` / ``db`` partials bitwise those of the plain add backward on the same ``s``; ``dres`` exactly
  +0 where dropped and within two bf16 roundings of ``c dx`` where kept;
* at T = 0 every output is bitwise the plain fused pair's;
* one captured graph draws fresh masks every replay and follows ``state.set`` with no re-capture;
* the gpt2_tiny executor program: bitwise the plain program at rate 0, one graph for every rate.

The shapes are the smallest at which these kernels can go wrong: one vector, rows that are no multiple of the waves
per workgroup, widths at and just past one vector per lane (512 / 520, 2048 / 2056), the widest each path takes, and
row counts one grid stride past the forward's and the backward's grid caps.
"""
import pytest
import torch

from polyaxon_amd.ops import _native
from polyaxon_amd.ops import dropout as dropout_mod
from polyaxon_amd.ops.dropout import DropoutState

pytestmark = pytest.mark.gpu

LN_SHAPES = [(1, 8), (5, 72), (7, 512), (7, 520), (9, 768), (6, 1024), (32771, 8), (4101, 64)]
RMS_SHAPES = [(1, 8), (3, 2048), (3, 2056), (2, 8192), (4099, 8), (1027, 8)]
CASES = [("ln", s) for s in LN_SHAPES] + [("rms", s) for s in RMS_SHAPES]
IDS = [f"{k}-{r}x{d}" for k, (r, d) in CASES]
RATES = [0, 6554, 32768, 65535]
KEY_SEED = (0x9E3779B9 << 32) | 0x85EBCA6B  # both key words non-zero, the first with its top bit set
STEP, SITE, EPS = 37, 5, 1e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _state(dev, T, step=STEP):
    st = DropoutState(dev, torch.full((1,), step, dtype=torch.int32, device=dev), seed=KEY_SEED)
    st.set(dropout=T / 65536.0)
    assert st.T == T and (st.hp.tolist()[0] & 0xFFFFFFFF) == T
    return st


def _mask(st, site, n_elem, step=None):
    """bool [n_elem] on the host: the contract's kept set of a tensor of n_elem elements (n_elem % 8 == 0)."""
    step = st.step() if step is None else step
    return torch.from_numpy(dropout_mod.mask_reference(st.key, step, site, n_elem // 8, st.T).reshape(-1))


def _rand(shape, dev, seed, nonzero=False):
    g = torch.Generator().manual_seed(seed)
    if nonzero:  # magnitude in [0.5, 2), random sign: no product with c in [1, 65536] is 0 or overflows bf16
        t = (torch.rand(shape, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    else:
        t = torch.randn(shape, generator=g)
    return t.to(torch.bfloat16).to(dev)


def _params(d, dev):
    g = torch.Generator().manual_seed(d)
    return ((1.0 + 0.25 * torch.randn(d, generator=g)).to(dev), (0.25 * torch.randn(d, generator=g)).to(dev))


def _forward(kind, x, res, w, b, st=None, site=SITE):
    """The fused add + norm forward through the native entry points: the drop pair with ``st``, the plain pair
    without.  Returns (s, y, mean or None, rstd)."""
    lib = _native.lib("plx_rms")
    rows, d = x.shape
    s, y = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    drop = () if st is None else (st.hp.data_ptr(), st.step_counter.data_ptr(), site)
    if kind == "ln":
        fn = lib.plx_add_ln_forward if st is None else lib.plx_add_ln_drop_forward
        rc = fn(x.data_ptr(), res.data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(), y.data_ptr(),
                mean.data_ptr(), rstd.data_ptr(), rows, d, EPS, *drop, _stream())
    else:
        mean = None
        fn = lib.plx_add_rms_forward if st is None else lib.plx_add_rms_drop_forward
        rc = fn(x.data_ptr(), res.data_ptr(), w.data_ptr(), s.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, d,
                EPS, *drop, _stream())
    assert rc == 0
    return s, y, mean, rstd


def _backward(kind, s, w, dy, mean, rstd, ds, st=None, site=SITE):
    """The fused backward.  Returns (dx, dres or None, partials [1 or 2, nb, d])."""
    lib = _native.lib("plx_rms")
    rows, d = s.shape
    dx = torch.empty_like(s)
    dres = None if st is None else torch.full_like(s, float("nan"))
    drop = () if st is None else (st.hp.data_ptr(), st.step_counter.data_ptr(), site)
    if kind == "ln":
        nb = lib.plx_ln_bwd_blocks(rows, d)
        part = torch.empty((2, nb, d), dtype=torch.float32, device=s.device)
        if st is None:
            rc = lib.plx_add_ln_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         ds.data_ptr(), dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), rows,
                                         d, _stream())
        else:
            rc = lib.plx_add_ln_drop_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(),
                                              rstd.data_ptr(), ds.data_ptr(), dx.data_ptr(), dres.data_ptr(),
                                              part[0].data_ptr(), part[1].data_ptr(), rows, d, *drop, _stream())
    else:
        nb = lib.plx_rms_bwd_blocks(rows)
        part = torch.empty((1, nb, d), dtype=torch.float32, device=s.device)
        if st is None:
            rc = lib.plx_add_rms_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(), ds.data_ptr(),
                                          dx.data_ptr(), part.data_ptr(), rows, d, _stream())
        else:
            rc = lib.plx_add_rms_drop_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(),
                                               ds.data_ptr(), dx.data_ptr(), dres.data_ptr(), part.data_ptr(), rows,
                                               d, *drop, _stream())
    assert rc == 0
    return dx, dres, part


def _plain_norm(kind, s, w, b):
    """(y, mean or None, rstd) of the existing unfused norm kernels on ``s``."""
    lib = _native.lib("plx_rms")
    rows, d = s.shape
    y = torch.empty_like(s)
    mean = torch.empty(rows, dtype=torch.float32, device=s.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=s.device)
    if kind == "ln":
        rc = lib.plx_ln_forward(s.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                rstd.data_ptr(), rows, d, EPS, _stream())
    else:
        mean = None
        rc = lib.plx_rms_forward(s.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, d, EPS, _stream())
    assert rc == 0
    return y, mean, rstd


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _scaled(t, c):
    """bf16(fp32(t) * c): the kept values of the contract, one fp32 product rounded once."""
    return (t.float() * torch.tensor(c, dtype=torch.float32, device=t.device)).to(torch.bfloat16)


# ------------------------------------------------------------------ 1. the mask, bit for bit
@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_forward_mask_is_the_reference(cuda, kind, shape, T):
    st = _state(cuda, T)
    w, b = _params(shape[1], cuda)
    res = _rand(shape, cuda, 1, nonzero=True)
    s, _, _, _ = _forward(kind, torch.zeros_like(res), res, w, b, st)
    torch.cuda.synchronize()
    keep = _mask(st, SITE, res.numel()).view(shape)
    s, want = s.cpu(), _scaled(res, st.c).cpu()
    assert torch.equal(s != 0, keep)
    assert torch.equal(_bits(s)[keep], _bits(want)[keep])
    assert bool((_bits(s)[~keep] == 0).all())  # +0, not -0


@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("n_vec", [1, 63, 64, 4097])
def test_standalone_pass_is_the_reference(cuda, n_vec, T):
    st = _state(cuda, T)
    x = _rand((n_vec * 8,), cuda, n_vec, nonzero=True)
    y = torch.full_like(x, float("nan"))
    rc = _native.lib("plx_rms").plx_dropout(x.data_ptr(), y.data_ptr(), n_vec, st.hp.data_ptr(),
                                            st.step_counter.data_ptr(), SITE, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    keep = _mask(st, SITE, x.numel())
    y, want = y.cpu(), _scaled(x, st.c).cpu()
    assert torch.equal(y != 0, keep)
    assert torch.equal(_bits(y)[keep], _bits(want)[keep]) and bool((_bits(y)[~keep] == 0).all())


def test_standalone_op_backward_redraws_the_mask(cuda):
    from polyaxon_amd.ops.rmsnorm import dropout

    st = _state(cuda, 32768)
    x = _rand((5, 24), cuda, 3, nonzero=True).requires_grad_()
    dy = _rand((5, 24), cuda, 4, nonzero=True)
    y = dropout(x, st, SITE)
    assert type(y.grad_fn).__name__ == "_DropoutBackward"
    (dx,) = torch.autograd.grad(y, x, dy)
    torch.cuda.synchronize()
    keep = _mask(st, SITE, x.numel()).view(5, 24)
    assert torch.equal(y.detach().cpu() != 0, keep) and torch.equal(dx.cpu() != 0, keep)
    assert _same(dx.cpu()[keep], _scaled(dy, st.c).cpu()[keep])


# ------------------------------------------------------------------ 2. values
@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_forward_values(cuda, kind, shape, T):
    """s against the fp64 ``ref = x + m c res``: |s - ref| <= 2^-8 |ref| + 2^-22 (|x| + |c res|) -- the half-ulp of
    the one bf16 rounding (8 significant bits) plus slack for the fp32 product and sum in front of it; y, mean and
    rstd bitwise the plain norm's on that s."""
    st = _state(cuda, T)
    w, b = _params(shape[1], cuda)
    x, res = _rand(shape, cuda, 5), _rand(shape, cuda, 6)
    s, y, mean, rstd = _forward(kind, x, res, w, b, st)
    y0, mean0, rstd0 = _plain_norm(kind, s, w, b)
    torch.cuda.synchronize()
    m = _mask(st, SITE, x.numel()).view(shape).double()
    xd, cres = x.cpu().double(), st.c * res.cpu().double()
    ref = xd + m * cres
    err = (s.cpu().double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * (xd.abs() + cres.abs())
    print(f"{kind} {shape} T={T}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert _same(y, y0) and _same(rstd, rstd0) and (mean is None or _same(mean, mean0))


# ------------------------------------------------------------------ 3. backward
@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_backward_passes_the_residual_gradient_through_the_mask(cuda, kind, shape, T):
    """dy = 0: the norm contributes nothing, so dx is ds bit for bit and dres is bf16(c ds) on the forward's kept
    set and +0 elsewhere."""
    st = _state(cuda, T)
    w, b = _params(shape[1], cuda)
    s, _, mean, rstd = _forward(kind, _rand(shape, cuda, 7), _rand(shape, cuda, 8), w, b, st)
    ds = _rand(shape, cuda, 9, nonzero=True)
    dx, dres, _ = _backward(kind, s, w, torch.zeros_like(s), mean, rstd, ds, st)
    torch.cuda.synchronize()
    keep = _mask(st, SITE, s.numel()).view(shape)
    assert _same(dx, ds)
    dres, want = dres.cpu(), _scaled(ds, st.c).cpu()
    assert torch.equal(dres != 0, keep)
    assert torch.equal(_bits(dres)[keep], _bits(want)[keep]) and bool((_bits(dres)[~keep] == 0).all())


# two bf16 roundings apart: dx = g (1 + e1) and dres = c g (1 + e32) (1 + e2) with |e1|, |e2| <= u = 2^-8 (bf16
# half-ulp) and |e32| <= 2^-24 (the fp32 product), so |dres - c dx| <= c |g| (2 u + 2^-24 + u 2^-24) and
# |g| <= |dx| / (1 - u)
U = 2.0 ** -8
TWO_ROUNDINGS = (2 * U + 2.0 ** -24 + U * 2.0 ** -24) / (1 - U)  # 1.004 x 2^-7


@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_backward_values(cuda, kind, shape, T):
    """Random dy and ds: dx and the dw / db partials bitwise the plain add backward's on the same s; dres exactly 0
    where dropped and within TWO_ROUNDINGS (derived above) of c dx where kept."""
    st = _state(cuda, T)
    w, b = _params(shape[1], cuda)
    s, _, mean, rstd = _forward(kind, _rand(shape, cuda, 10), _rand(shape, cuda, 11), w, b, st)
    dy, ds = _rand(shape, cuda, 12), _rand(shape, cuda, 13)
    dx, dres, part = _backward(kind, s, w, dy, mean, rstd, ds, st)
    dx0, _, part0 = _backward(kind, s, w, dy, mean, rstd, ds)
    torch.cuda.synchronize()
    assert _same(dx, dx0) and _same(part, part0)
    keep = _mask(st, SITE, s.numel()).view(shape)
    dres = dres.cpu()
    assert bool((_bits(dres)[~keep] == 0).all())
    cdx = st.c * dx.cpu().double()
    err = (dres.double() - cdx).abs()[keep]
    bound = TWO_ROUNDINGS * cdx.abs()[keep]
    if err.numel():
        print(f"{kind} {shape} T={T}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


def test_backward_without_a_residual_gradient(cuda):
    """ds = None (the last norm of the model): the plain norm backward's dx, dropped out for the branch."""
    lib = _native.lib("plx_rms")
    for kind, shape in (("ln", (9, 768)), ("rms", (3, 2056))):
        st = _state(cuda, 6554)
        w, b = _params(shape[1], cuda)
        s, _, mean, rstd = _forward(kind, _rand(shape, cuda, 14), _rand(shape, cuda, 15), w, b, st)
        dy = _rand(shape, cuda, 16)
        rows, d = shape
        dx, dres, dx0 = torch.empty_like(s), torch.empty_like(s), torch.empty_like(s)
        if kind == "ln":
            nb = lib.plx_ln_bwd_blocks(rows, d)
            part, part0 = (torch.empty((2, nb, d), dtype=torch.float32, device=cuda) for _ in range(2))
            assert lib.plx_add_ln_drop_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(),
                                                rstd.data_ptr(), None, dx.data_ptr(), dres.data_ptr(),
                                                part[0].data_ptr(), part[1].data_ptr(), rows, d, st.hp.data_ptr(),
                                                st.step_counter.data_ptr(), SITE, _stream()) == 0
            assert lib.plx_ln_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                       dx0.data_ptr(), part0[0].data_ptr(), part0[1].data_ptr(), rows, d,
                                       _stream()) == 0
        else:
            nb = lib.plx_rms_bwd_blocks(rows)
            part, part0 = (torch.empty((1, nb, d), dtype=torch.float32, device=cuda) for _ in range(2))
            assert lib.plx_add_rms_drop_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(), None,
                                                 dx.data_ptr(), dres.data_ptr(), part.data_ptr(), rows, d,
                                                 st.hp.data_ptr(), st.step_counter.data_ptr(), SITE, _stream()) == 0
            assert lib.plx_rms_backward(s.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(), dx0.data_ptr(),
                                        part0.data_ptr(), rows, d, _stream()) == 0
        torch.cuda.synchronize()
        assert _same(dx, dx0) and _same(part, part0)
        keep = _mask(st, SITE, s.numel()).view(shape)
        dres = dres.cpu()
        assert bool((_bits(dres)[~keep] == 0).all())
        cdx = st.c * dx.cpu().double()
        assert bool(((dres.double() - cdx).abs()[keep] <= TWO_ROUNDINGS * cdx.abs()[keep]).all())


# ------------------------------------------------------------------ 4. T = 0 is the plain pair
@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_bitwise_the_plain_pair_at_zero(cuda, kind, shape):
    st = _state(cuda, 0)
    w, b = _params(shape[1], cuda)
    x, res = _rand(shape, cuda, 17), _rand(shape, cuda, 18)
    dy, ds = _rand(shape, cuda, 19), _rand(shape, cuda, 20)
    s, y, mean, rstd = _forward(kind, x, res, w, b, st)
    s0, y0, mean0, rstd0 = _forward(kind, x, res, w, b)
    dx, dres, part = _backward(kind, s, w, dy, mean, rstd, ds, st)
    dx0, _, part0 = _backward(kind, s0, w, dy, mean0, rstd0, ds)
    torch.cuda.synchronize()
    assert _same(s, s0) and _same(y, y0) and _same(rstd, rstd0) and (mean is None or _same(mean, mean0))
    assert _same(dx, dx0) and _same(dres, dx0) and _same(part, part0)


# ------------------------------------------------------------------ 5. entry points
def test_entry_points_reject_what_they_do_not_take(cuda):
    lib = _native.lib("plx_rms")
    st = _state(cuda, 6554)
    hp, step = st.hp.data_ptr(), st.step_counter.data_ptr()
    for rows, d, h, t in ((4, 12, hp, step), (4, 1032, hp, step), (0, 64, hp, step), (-1, 64, hp, step),
                          (4, 64, None, step), (4, 64, hp, None)):
        assert lib.plx_add_ln_drop_forward(0, 0, 0, 0, 0, 0, 0, 0, rows, d, EPS, h, t, 0, _stream()) == 1
        assert lib.plx_add_ln_drop_backward(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, rows, d, h, t, 0, _stream()) == 1
    for rows, d, h, t in ((4, 12, hp, step), (4, 8200, hp, step), (0, 64, hp, step), (4, 64, None, step),
                          (4, 64, hp, None)):
        assert lib.plx_add_rms_drop_forward(0, 0, 0, 0, 0, 0, rows, d, EPS, h, t, 0, _stream()) == 1
        assert lib.plx_add_rms_drop_backward(0, 0, 0, 0, 0, 0, 0, 0, rows, d, h, t, 0, _stream()) == 1
    for n, h, t in ((0, hp, step), (-8, hp, step), (8, None, step), (8, hp, None)):
        assert lib.plx_dropout(0, 0, n, h, t, 0, _stream()) == 1
    torch.cuda.synchronize()


def test_without_drop_the_ops_are_the_plain_functions(cuda):
    from polyaxon_amd.ops import rmsnorm

    w, b = _params(72, cuda)
    x, res = (_rand((5, 72), cuda, 21 + i).requires_grad_() for i in range(2))
    st = _state(cuda, 6554)
    names = [type(f(x, res)[0].grad_fn).__name__ for f in (
        lambda x, r: rmsnorm.add_layer_norm(x, r, w, b), lambda x, r: rmsnorm.add_rms_norm(x, r, w),
        lambda x, r: rmsnorm.add_layer_norm(x, r, w, b, drop=(st, 1)),
        lambda x, r: rmsnorm.add_rms_norm(x, r, w, drop=(st, 1)))]
    assert names == ["_AddLayerNormBackward", "_AddRMSNormBackward", "_AddLayerNormDropBackward",
                     "_AddRMSNormDropBackward"]


def test_wide_layer_norm_takes_the_standalone_pass(cuda):
    """add + LayerNorm above d = 1024 has no fused pair: the branch goes through plx_dropout, then the plain add and
    norm -- the same kept set."""
    from polyaxon_amd.ops import rmsnorm

    shape = (3, 1032)
    st = _state(cuda, 32768)
    w, b = _params(shape[1], cuda)
    res = _rand(shape, cuda, 23, nonzero=True).requires_grad_()
    x = torch.zeros(shape, dtype=torch.bfloat16, device=cuda)
    s, y = rmsnorm.add_layer_norm(x, res, w, b, drop=(st, SITE))
    (dres,) = torch.autograd.grad(s, res, torch.ones_like(s))
    torch.cuda.synchronize()
    keep = _mask(st, SITE, res.numel()).view(shape)
    assert torch.equal(s.detach().cpu() != 0, keep) and torch.equal(dres.cpu() != 0, keep)
    assert _same(y.detach(), rmsnorm.layer_norm(s.detach(), w, b))


# ------------------------------------------------------------------ 6. one captured graph
def test_one_captured_graph_draws_fresh_masks_and_follows_the_rate(cuda):
    """Forward + backward of add_layer_norm(drop=...) and the step increment captured once: every replay drops the
    reference's set of its own step, and after state.set the same graph computes the new rate's outputs, bit for bit
    the eager ones."""
    from polyaxon_amd.ops.rmsnorm import add_layer_norm

    shape = (9, 768)
    st = _state(cuda, 6554, step=0)
    step = st.step_counter
    w, b = (p.requires_grad_() for p in _params(shape[1], cuda))
    x = torch.zeros(shape, dtype=torch.bfloat16, device=cuda).requires_grad_()
    res = _rand(shape, cuda, 24, nonzero=True).requires_grad_()
    ds, dy = _rand(shape, cuda, 25, nonzero=True), torch.zeros(shape, dtype=torch.bfloat16, device=cuda)

    def fwd_bwd():
        s, y = add_layer_norm(x, res, w, b, EPS, drop=(st, SITE))
        dx, dres = torch.autograd.grad([s, y], [x, res], [ds, dy])
        return s.detach(), y.detach(), dx, dres

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        fwd_bwd()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fwd_bwd()
        step += 1
    step.zero_()
    seen = []
    for t, T in ((0, 6554), (1, 6554), (2, 6554), (3, 32768), (4, 0)):
        if T != st.T:
            st.set(dropout=T / 65536.0)
        graph.replay()
        got = [o.clone() for o in static]
        torch.cuda.synchronize()
        assert int(step.item()) == t + 1
        keep = _mask(st, SITE, x.numel(), step=t).view(shape)
        assert torch.equal(got[0].cpu() != 0, keep) and torch.equal(got[3].cpu() != 0, keep)
        step.fill_(t)
        want = fwd_bwd()
        step.fill_(t + 1)
        torch.cuda.synchronize()
        for a, e in zip(got, want):
            assert _same(a, e)
        seen.append(keep)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])  # fresh bits every replay
    assert bool(seen[4].all())


# ------------------------------------------------------------------ 7. the executor
def test_executor_searches_dropout_in_one_captured_step(cuda, monkeypatch):
    from polyaxon_amd.ops import rmsnorm
    from polyaxon_amd.polyflow.programs import build_program

    calls = []
    lib = _native.lib("plx_rms")
    fwd = lib.plx_add_ln_drop_forward
    monkeypatch.setattr(lib, "plx_add_ln_drop_forward", lambda *a: (calls.append(a[-2]), fwd(*a))[1])
    monkeypatch.setattr(rmsnorm, "drop_factor", lambda *a: pytest.fail("the torch fallback ran"))

    params = {"graph": True}
    plain = build_program("gpt2_tiny", dict(params), cuda)
    plain.warm()
    if plain.executor.graph is None:
        print("the plain gpt2_tiny capture was rejected here: both programs run eager")
        params = {"graph": False}
        plain = build_program("gpt2_tiny", dict(params), cuda)
        plain.warm()
    assert not calls  # feature off: not one drop launch
    prog = build_program("gpt2_tiny", dict(params, dropout=True), cuda)
    assert prog.hp_keys == plain.hp_keys + ("dropout",)
    prog.warm()
    ex0, ex = plain.executor, prog.executor
    assert (ex.graph is None) == (ex0.graph is None) and ex0.dropout is None
    n_layers = ex.model.cfg.n_layers
    assert set(calls) == set(range(2 * n_layers))  # the fused kernel at every residual site, in the captured step
    graph = ex.graph
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k != "dropout"}

    def trial(e, c0, seed, steps, **hp):
        e.data.counter.copy_(c0)  # the token stream's own counter: every trial reads the same batches
        e.reset(seed=seed)
        e.set_hparams(**base, **hp)
        e.run(steps)
        torch.cuda.synchronize()
        return e.flat.params.clone(), float(e.losses()[0])

    c0 = ex0.data.counter.clone()
    p0, l0 = trial(ex0, c0, 3, 3, dropout=0.3)  # no param: the key is dropped
    p, l = trial(ex, c0, 3, 3, dropout=0.0)
    assert torch.equal(p, p0) and l == l0          # rate 0: bitwise the plain program
    q, _ = trial(ex, c0, 3, 3, dropout=0.3)
    assert ex.graph is graph                       # the same captured step
    assert not torch.equal(q, p) and bool(torch.isfinite(q).all())
    q2, _ = trial(ex, c0, 3, 3, dropout=0.3)
    assert torch.equal(q2, q)
