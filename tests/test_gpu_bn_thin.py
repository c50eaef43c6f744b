"""The thinned BatchNorm kernels (``PLX_BN_THIN=1``, csrc/bn_kernels.hip ``*_thin_kernel``) against the kernels they
replace (``PLX_BN_THIN=0``): every output must be bit-identical (``torch.equal``), in one process, through
``plx_bn_set_thin``, on identical inputs.  Every output lives between sentinel-filled margins that must stay
untouched, and every case runs twice per setting and must repeat itself exactly.

Loop coverage of the new kernels:

* forward (``stem_apply_pool_thin_kernel``): one loop, down the ``kStemFwdRows`` = 8 output rows of a block.
  (3, 15, 13, 64) has OH = 8 (8 trips), (2, 32, 34, 16) has OH = 16 (two full row chunks per image), (1, 7, 9, 8) has
  OH = 4 and (128, 66, 6, 64) has OH = 33 (ragged last chunks of 4 and 1 trips); the one- and two-row images run the
  prologue with a single trip.
* stem dx (``stem_pool_bn_bwd_thin_kernel<true>``): one loop over the ``kStemDxRows`` = 4 quad rows of a block.
  (2, 8, 8, 64) has 8 quad rows (2 blocks of 4 trips), (3, 3, 5, 8) has 6 (a full block, then a ragged one of 2 trips),
  (1, 1, 1, 64) and (1, 2, 3, 64) have 1 (a ragged single trip).
* stem partials (``stem_pool_bn_bwd_thin_kernel<false>``): the grid-stride loop over quad rows it shares with its
  predecessor; (128, 66, 6, 64) has 4224 quad rows on 4096 blocks: a second trip for the first 128, none for the rest.
* both stem backward kernels stage their NA x C constants (NA = 5 for dx, 4 for the partials) with a loop over 256
  threads: C = 64 gives 320 (two trips, the second ragged) and 256 (one full trip), C = 8 and 16 a ragged single trip.
* residual-BatchNorm dx: its thinned kernel did not beat ``bn_bwd_dx_kernel<true, *, *>`` alone or in the step
  (``profiles/bn_thin.md``) and was removed, so one kernel serves both settings; the cases stay as the guard for a
  later attempt: (4200, 2048) has 1,075,200 vectors on 4096 x 256 threads (a second, ragged grid-stride trip), (37, 64)
  and (1000, 256) leave the last block partly idle.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 64  # elements on either side of every output (a multiple of 16 bytes for every dtype used)
SENTINEL = {torch.bfloat16: -7.0, torch.float32: -12345.0, torch.uint8: 0xA5}

STEM_FWD_SHAPES = [(1, 1, 1, 64), (1, 2, 3, 64), (1, 7, 9, 8), (2, 8, 8, 64), (3, 15, 13, 64), (2, 32, 34, 16),
                   (3, 3, 5, 8)]
STEM_BWD_SHAPES = STEM_FWD_SHAPES + [(128, 66, 6, 64)]
RES_SHAPES = [(37, 64), (1000, 256), (4200, 2048)]


class Guarded:
    """A tensor of ``numel`` elements with PAD sentinel elements before and after it."""

    def __init__(self, numel, dtype, dev, fill=None):
        self.all = torch.full((numel + 2 * PAD,), SENTINEL[dtype], dtype=dtype, device=dev)
        self.t = self.all[PAD:PAD + numel]
        if fill is not None:
            self.t.copy_(fill)
        self.ptr = self.t.data_ptr()

    def check(self):
        s = torch.full((PAD,), SENTINEL[self.all.dtype], dtype=self.all.dtype, device=self.all.device)
        assert torch.equal(self.all[:PAD], s) and torch.equal(self.all[-PAD:], s), "a kernel wrote outside its output"
        return self.t


def _lib():
    from polyaxon_amd.ops import _native

    return _native.lib("plx_bn")


def _env(dev):
    from polyaxon_amd.ops.bn_fused import _counters, _stream

    return _counters(dev), _stream()


@pytest.fixture(autouse=True)
def _restore_switch():
    yield
    _lib().plx_bn_set_thin(1)


def _stem_inputs(shape, dev):
    n, h, w, c = shape
    gen = torch.Generator(device="cpu").manual_seed(1234 + n * 1000 + h * 100 + w * 10 + c)
    # a handful of values, so that windows hold exact ties; a block of strongly negative pixels on top
    x = (torch.randint(-3, 4, (n, h, w, c), generator=gen).float() * 0.5)
    x[:, : max(1, h // 2), : max(1, w // 2)] -= 4.0
    x = x.to(torch.bfloat16).to(dev)
    gamma = torch.rand(c, generator=gen) + 0.5
    gamma[0::4] = 0.0          # zero: the whole channel is relu(beta), all ties
    gamma[1::4] *= -1.0        # negative: the order of the values flips
    beta = torch.randn(c, generator=gen) * 0.3
    beta[0::8] = -1.0          # with gamma = 0: every tap is 0 after ReLU, the first valid tap must win
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = (torch.randint(-4, 5, (n, oh, ow, c), generator=gen).float() * 0.25).to(torch.bfloat16).to(dev)
    return x, gamma.to(dev), beta.to(dev), dy


def _stem_forward(lib, thin, shape, x, gamma, beta):
    n, h, w, c = shape
    dev = x.device
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    lib.plx_bn_set_thin(thin)
    cnt, st = _env(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    y = Guarded(n * oh * ow * c, torch.bfloat16, dev)
    idx = Guarded(n * oh * ow * c, torch.uint8, dev)
    stats = torch.empty(4 * c, **f32)  # mean | invstd | scale | bias
    ws = torch.empty(int(lib.plx_bn_workspace(n * h * w, c)), **f32)
    rm, rv = torch.zeros(c, **f32), torch.ones(c, **f32)
    rc = lib.plx_stem_bn_pool_forward(x.data_ptr(), y.ptr, idx.ptr, n, h, w, c, gamma.data_ptr(), beta.data_ptr(),
                                      1e-5, 0.1, rm.data_ptr(), rv.data_ptr(), stats.data_ptr(), stats[c:].data_ptr(),
                                      stats[2 * c:].data_ptr(), ws.data_ptr(), None, 0, cnt, st)
    assert rc == 0
    torch.cuda.synchronize()
    return y.check(), idx.check(), stats


def _stem_backward(lib, thin, shape, x, gamma, dy, idx, stats, grads0):
    n, h, w, c = shape
    dev = x.device
    lib.plx_bn_set_thin(thin)
    cnt, st = _env(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    dx = Guarded(n * h * w * c, torch.bfloat16, dev)
    dgamma = Guarded(c, torch.float32, dev, fill=grads0[0] if grads0 is not None else None)
    dbeta = Guarded(c, torch.float32, dev, fill=grads0[1] if grads0 is not None else None)
    coef = Guarded(3 * c, torch.float32, dev)
    ws = Guarded(int(lib.plx_stem_bn_pool_bwd_workspace(n, h, w, c)), torch.float32, dev)
    rc = lib.plx_stem_bn_pool_backward(dy.data_ptr(), idx.data_ptr(), x.data_ptr(), dx.ptr, n, h, w, c,
                                       gamma.data_ptr(), stats.data_ptr(), stats[c:].data_ptr(),
                                       stats[2 * c:].data_ptr(), dgamma.ptr, dbeta.ptr, coef.ptr, ws.ptr,
                                       1 if grads0 is not None else 0, cnt, st)
    assert rc == 0
    torch.cuda.synchronize()
    ws.check()
    return dx.check(), dgamma.check(), dbeta.check(), coef.check()


_STEM_FWD = {}


def _stem_forward_all(shape, dev):
    """x, gamma, beta, dy and the forward's four runs (off, off, on, on), computed once per shape."""
    if shape not in _STEM_FWD:
        lib = _lib()
        x, gamma, beta, dy = _stem_inputs(shape, dev)
        runs = [_stem_forward(lib, thin, shape, x, gamma, beta) for thin in (0, 0, 1, 1)]
        _STEM_FWD[shape] = (x, gamma, beta, dy, runs)
    return _STEM_FWD[shape]


@pytest.mark.parametrize("shape", STEM_BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_forward_bit_identical(cuda, shape):
    x, gamma, beta, dy, runs = _stem_forward_all(shape, cuda)
    y0, i0, s0 = runs[0]
    assert int(i0.max()) <= 8, "every output has a window position"
    for y, i, s in runs[1:]:
        assert torch.equal(y, y0)
        assert torch.equal(i, i0)
        assert torch.equal(s, s0)
    # the inputs do what they are meant to: exact ties exist, and some windows are all zero after the ReLU
    assert int((y0.float() == 0).sum()) > 0


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("shape", STEM_BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_backward_bit_identical(cuda, shape, accumulate):
    lib = _lib()
    x, gamma, beta, dy, runs = _stem_forward_all(shape, cuda)
    _, idx, stats = runs[0]
    c = shape[3]
    grads0 = None
    if accumulate:
        gen = torch.Generator(device="cpu").manual_seed(7)
        grads0 = (torch.randn(c, generator=gen).to(cuda), torch.randn(c, generator=gen).to(cuda))
    outs = [_stem_backward(lib, thin, shape, x, gamma, dy, idx, stats, grads0) for thin in (0, 0, 1, 1)]
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0].float()).all())


def _res_inputs(m, c, dev):
    gen = torch.Generator(device="cpu").manual_seed(99 + m + c)
    f32 = dict(dtype=torch.float32)
    t = {}
    for name in ("x", "dy", "x2"):
        t[name] = torch.randn(m, c, generator=gen).to(torch.bfloat16).to(dev)
    for name in ("mask", "mask2"):
        t[name] = torch.randint(0, 256, (m * c // 8,), generator=gen, dtype=torch.int32).to(torch.uint8).to(dev)
    for name in ("gamma", "gamma2"):
        t[name] = (torch.rand(c, generator=gen, **f32) + 0.5).to(dev)
    for name in ("mean", "mean2"):
        t[name] = (torch.randn(c, generator=gen, **f32) * 0.2).to(dev)
    for name in ("invstd", "invstd2"):
        t[name] = (torch.rand(c, generator=gen, **f32) + 0.5).to(dev)
    return t


def _res_backward(lib, thin, m, c, t, relu, rmask):
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import bn_backward

    dev = t["x"].device
    lib.plx_bn_set_thin(thin)
    cnt, st = _env(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    nblk2 = int(lib.plx_bn_dx_blocks(m, c))
    dx = Guarded(m * c, torch.bfloat16, dev)
    dres = Guarded(m * c, torch.bfloat16, dev)
    part = Guarded(2 * nblk2 * c, torch.float32, dev)
    dgb = torch.empty(2 * c, **f32)
    coef = torch.empty(3 * c, **f32)
    ws = torch.empty(int(lib.plx_bn_workspace(m, c)), **f32)
    rb = _native.ResBnArgs(t["x2"].data_ptr(), t["mask2"].data_ptr() if rmask else None, t["mean2"].data_ptr(),
                           t["invstd2"].data_ptr(), part.ptr)
    bn_backward(x=t["x"], mask=t["mask"] if relu else None, dy=t["dy"], dx=dx.ptr, dres=dres.ptr, m=m, c=c,
                gamma=t["gamma"], save_mean=t["mean"], save_invstd=t["invstd"], dgamma=dgb, dbeta=dgb[c:], coef=coef,
                workspace=ws, relu=relu, accumulate=0, resbn=rb, counters=cnt, stream=st)
    # the residual BatchNorm's backward from those partials (no reduce pass of its own)
    dx2 = Guarded(m * c, torch.bfloat16, dev)
    dgb2 = Guarded(2 * c, torch.float32, dev)
    coef2 = torch.empty(3 * c, **f32)
    l2 = torch.empty(int(lib.plx_bn_l2_workspace(nblk2, c)), **f32)
    bn_backward(x=t["x2"], mask=t["mask2"] if rmask else None, dy=dres.ptr, dx=dx2.ptr, m=m, c=c, gamma=t["gamma2"],
                save_mean=t["mean2"], save_invstd=t["invstd2"], dgamma=dgb2.ptr, dbeta=dgb2.t[c:], coef=coef2,
                ext_part=part.ptr, ext_nblk=nblk2, workspace=l2, relu=rmask, accumulate=0, counters=cnt, stream=st)
    torch.cuda.synchronize()
    return dx.check(), dres.check(), part.check(), dgb2.check(), dx2.check()


@pytest.mark.parametrize("rmask", [False, True], ids=["res_plain", "res_relu"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("m,c", RES_SHAPES)
def test_residual_bn_dx_bit_identical(cuda, m, c, relu, rmask):
    lib = _lib()
    t = _res_inputs(m, c, cuda)
    outs = [_res_backward(lib, thin, m, c, t, relu, rmask) for thin in (0, 0, 1, 1)]
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][3]).all())
