"""GPU tests of label smoothing and z-loss as device-resident loss hyper-parameters: the plx_xent_hp_* /
plx_xent_cls_hp_* kernels (csrc/lm_kernels.hip) against float64 per row and per element, bitwise against the plain
pair at zero, inside a captured graph, and through the resident executor (ops/loss_hp.py, ops/lm.py,
polyflow/executor.py) on a real MI355X.

Where the bounds come from
--------------------------
Forward, per row: |got - ref| <= FWD_C * (|l| + |x_t| + eps * mean_{j<C}|x_j| + zeta * l^2), FWD_C = 2e-5, for each of
lse, loss and nll (ref in float64 from the same bf16 logits).

* The log-sum-exp: a lane walks the row's 16-byte chunks 4 at a time.  At V = 50432 a row is 6304 chunks over 256
  lanes: at most 25 chunks = 200 elements per lane (197 when counted in elements), summed after their ``__expf``;
  every trip of 4 chunks is folded into the running (max, sum) by two multiplies and an add (7 trips: 21 roundings),
  then 6 wave-shuffle levels and 3 LDS steps of the same three operations (27).  That is about 248 fp32 roundings
  of 2^-24 on the longest path, all terms positive: 1.5e-5 relative on the sum, which is 1.5e-5 absolute on l =
  m + log(sum); ``__expf`` / ``__logf`` add a few 1e-7.  2e-5 covers it, and |l| + |x_t| is at least ~1 on every row
  below (l >= max_j x_j, logits ~ 3 N(0, 1)), so the scaled bound is no tighter than the absolute one.
* The smoothing term: the same walk adds x_j (j < C) per lane (200), then 6 shuffle levels and 3 LDS adds: 209
  roundings, each at most 2^-24 of sum |x_j|: 1.25e-5 * mean|x_j| on the mean, times eps in the loss.
* zeta l^2 inherits 2 zeta |l| times the error of l and one rounding of its own: below 2e-5 zeta l^2 for |l| >= 1.5.

Backward, per element: |got - ref| <= 2^-8 |ref| + BWD_C * |g| * row_scale, BWD_C = 2e-5, g = dloss / rows the
incoming scale, row_scale = 1 + 2 zeta |l| the largest magnitude a term of p (1 + 2 zeta l) - (1 - eps)[j = t] -
(eps / C)[j < C] can take.  The first term is the one bf16 rounding of the result: bf16 keeps 8 significant bits, so
round-to-nearest is off by at most 2^-8 of the value (half an ulp of 2^-7) -- that term carries no margin of its own.
The second is the fp32 error of p = exp(x - l) -- relative 1.5e-5 from l as above plus ``__expf``'s, in fact a few
1e-7 on these rows -- and of the cancellation against the two constants, which rounds at 2^-24 of the same
magnitude; the margin of the whole bound is there (observed worst ratios 0.2 .. 0.93, set by the bf16 rounding).
"""
import functools

import pytest
import torch

from polyaxon_amd.ops import _native

pytestmark = pytest.mark.gpu

FWD_C = 2e-5
BWD_C = 2e-5
DLOSS = 1.7
HPS = [(0.0, 0.0), (0.1, 0.0), (0.0, 1e-3), (0.2, 1e-4)]
LM_SHAPES = [
    (1, 2, 7, 7),            # a row shorter than one chunk
    (2, 5, 1001, 1001),      # odd V: rows start mid-chunk, both edge chunks partial
    (2, 3, 264, 257),        # C inside the last chunks, -inf padding
    (1, 3, 8200, 8200),      # a second 4 x 256-chunk trip with a ragged end
    (2, 3, 50432, 50257),    # GPT-2's real padding
]
CLS_SHAPES = [(1, 7, 7), (3, 1001, 1001), (8, 264, 257), (2, 8200, 8200)]
CASES = [("lm", s) for s in LM_SHAPES] + [("cls", s) for s in CLS_SHAPES]
IDS = ["-".join([k] + [str(d) for d in s]) for k, s in CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    """Inputs of one shape and everything of the float64 reference that does not depend on (eps, zeta); computed once
    and shared (nothing below writes into it).  Rows are the loss rows: (b, s < S - 1) or the N classification rows."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(sum(shape))
    *lead, V, C = shape
    logits = (torch.randn(*lead, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    logits[..., C:] = float("-inf")
    targets = torch.randint(0, C, tuple(lead), device=dev, generator=g)
    if kind == "lm":
        B, S = lead
        if B * (S - 1) >= 3:
            targets[0, 1] = -100                          # ignore_index
            targets[-1, S - 1] = C if C < V else V + 5    # a label in the padding [C, V), or past the row
        x = logits[:, :-1].reshape(-1, V).double()
        t = targets[:, 1:].reshape(-1)
    else:
        (N,) = lead
        if N >= 3:
            targets[1] = -100
        if N >= 8:
            targets[5] = C + 2 if C < V else V
        x = logits.double()
        t = targets
    valid = (t >= 0) & (t < C)
    l = torch.logsumexp(x, dim=-1)
    xt = x.gather(1, torch.where(valid, t, torch.zeros_like(t))[:, None])[:, 0]
    return {"logits": logits, "targets": targets, "x": x, "t": t, "valid": valid, "l": l, "xt": xt,
            "sbar": x[:, :C].mean(-1), "sabs": x[:, :C].abs().mean(-1), "rows": x.shape[0]}


def _lhp(eps, zeta):
    return torch.tensor([eps, zeta, 0.0, 0.0], dtype=torch.float32, device="cuda")


def _forward(kind, shape, lhp, hp=True):
    """lse, loss(, nll) rows straight from the C entry points; every output starts as NaN."""
    lib = _native.lib("plx_lm")
    c = _case(kind, shape)
    *lead, V, C = shape
    out = [torch.full((c["rows"],), float("nan"), device="cuda") for _ in range(3 if hp else 2)]
    lg, tg = c["logits"], c["targets"]
    if kind == "lm" and hp:
        rc = lib.plx_xent_hp_fwd(lg.data_ptr(), tg.data_ptr(), lhp.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                 out[2].data_ptr(), lead[0], lead[1], V, C, _stream())
    elif kind == "lm":
        rc = lib.plx_xent_fwd(lg.data_ptr(), tg.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), lead[0], lead[1], V,
                              _stream())
    elif hp:
        rc = lib.plx_xent_cls_hp_fwd(lg.data_ptr(), tg.data_ptr(), lhp.data_ptr(), out[0].data_ptr(),
                                     out[1].data_ptr(), out[2].data_ptr(), lead[0], V, C, _stream())
    else:
        rc = lib.plx_xent_cls_fwd(lg.data_ptr(), tg.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), lead[0], V,
                                  _stream())
    _native.check(rc, "xent forward")
    return out


def _backward(kind, shape, lse, lhp, hp=True):
    """The bf16 logits gradient from the C entry points for an incoming gradient of DLOSS; starts as NaN."""
    lib = _native.lib("plx_lm")
    c = _case(kind, shape)
    *lead, V, C = shape
    lg, tg = c["logits"], c["targets"]
    grad = torch.full_like(lg, float("nan"))
    dloss = torch.tensor([DLOSS], dtype=torch.float32, device="cuda")
    if kind == "lm" and hp:
        rc = lib.plx_xent_hp_bwd(lg.data_ptr(), tg.data_ptr(), lse.data_ptr(), lhp.data_ptr(), dloss.data_ptr(),
                                 grad.data_ptr(), lead[0], lead[1], V, C, _stream())
    elif kind == "lm":
        rc = lib.plx_xent_bwd(lg.data_ptr(), tg.data_ptr(), lse.data_ptr(), dloss.data_ptr(), grad.data_ptr(),
                              lead[0], lead[1], V, _stream())
    elif hp:
        rc = lib.plx_xent_cls_hp_bwd(lg.data_ptr(), tg.data_ptr(), lse.data_ptr(), lhp.data_ptr(), dloss.data_ptr(),
                                     grad.data_ptr(), lead[0], V, C, 0.0, _stream())
    else:
        rc = lib.plx_xent_cls_bwd(lg.data_ptr(), tg.data_ptr(), lse.data_ptr(), dloss.data_ptr(), grad.data_ptr(),
                                  lead[0], V, 0.0, _stream())
    _native.check(rc, "xent backward")
    return grad


@pytest.mark.parametrize("eps,zeta", HPS)
@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_forward_rows_match_float64(cuda, kind, shape, eps, zeta):
    c = _case(kind, shape)
    lse, loss, nll = _forward(kind, shape, _lhp(eps, zeta))
    torch.cuda.synchronize()
    l, xt, valid = c["l"], c["xt"], c["valid"]
    zero = torch.zeros_like(l)
    ref_nll = torch.where(valid, l - xt, zero)
    ref_loss = torch.where(valid, l - (1 - eps) * xt - eps * c["sbar"] + zeta * l * l, zero)
    bound = FWD_C * (l.abs() + xt.abs() + eps * c["sabs"] + zeta * l * l)
    worst = 0.0
    for name, got, ref in (("lse", lse, l), ("loss", loss, ref_loss), ("nll", nll, ref_nll)):
        err = (got.double() - ref).abs()
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print(f"{kind} {shape} eps={eps} zeta={zeta} {name}: worst error / bound = {ratio:.3g}")
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (name, ratio)
    print(f"{kind} {shape} eps={eps} zeta={zeta}: worst ratio {worst:.3g}")
    if not bool(valid.all()):  # ignored rows: exactly nothing
        assert float(loss[~valid].abs().max()) == 0.0 and float(nll[~valid].abs().max()) == 0.0
    if eps == 0.0 and zeta == 0.0:
        assert torch.equal(nll, loss)


@pytest.mark.parametrize("eps,zeta", HPS)
@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_backward_elements_match_float64(cuda, kind, shape, eps, zeta):
    c = _case(kind, shape)
    *lead, V, C = shape
    lhp = _lhp(eps, zeta)
    lse = _forward(kind, shape, lhp)[0]
    grad = _backward(kind, shape, lse, lhp)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all())  # every element was written
    g = DLOSS / c["rows"]
    x, l, t, valid = c["x"], c["l"], c["t"], c["valid"]
    cols = torch.arange(V, device=x.device)
    ref = torch.exp(x - l[:, None]) * (1 + 2 * zeta * l)[:, None]
    ref = ref - (1 - eps) * (cols[None, :] == t[:, None]) - (eps / C) * (cols < C)[None, :]
    ref = torch.where(valid[:, None], ref * g, torch.zeros_like(ref))
    if kind == "lm":
        got = grad[:, :-1].reshape(-1, V)
        assert float(grad[:, -1].float().abs().max()) == 0.0  # the last position predicts nothing
    else:
        got = grad
    got = got.double()
    bound = ref.abs() * 2.0 ** -8 + BWD_C * abs(g) * (1 + 2 * zeta * l.abs())[:, None]
    err = (got - ref).abs()
    print(f"{kind} {shape} eps={eps} zeta={zeta} grad: worst error / bound = {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    if not bool(valid.all()):  # -100, a label in [C, V) or past the row: zero rows
        assert float(got[~valid].abs().max()) == 0.0
    if zeta == 0.0 and C < V:  # the padding columns of valid rows take no gradient
        assert float(got[valid][:, C:].abs().max()) == 0.0


@pytest.mark.parametrize("kind,shape", [c for c in CASES if c[1][-1] == c[1][-2]],
                         ids=[i for i, c in zip(IDS, CASES) if c[1][-1] == c[1][-2]])
def test_bitwise_the_plain_pair_at_zero(cuda, kind, shape):
    lhp = _lhp(0.0, 0.0)
    lse, loss, nll = _forward(kind, shape, lhp)
    lse0, loss0 = _forward(kind, shape, None, hp=False)
    grad = _backward(kind, shape, lse, lhp)
    grad0 = _backward(kind, shape, lse0, None, hp=False)
    torch.cuda.synchronize()
    assert torch.equal(lse, lse0) and torch.equal(loss, loss0) and torch.equal(nll, loss)
    assert torch.equal(grad.view(torch.int16), grad0.view(torch.int16))


def test_entry_points_reject_bad_class_counts(cuda):
    lib = _native.lib("plx_lm")
    for C in (0, 9, -1):
        assert lib.plx_xent_hp_fwd(0, 0, 0, 0, 0, 0, 1, 2, 8, C, _stream()) == 1
        assert lib.plx_xent_hp_bwd(0, 0, 0, 0, 0, 0, 1, 2, 8, C, _stream()) == 1
        assert lib.plx_xent_cls_hp_fwd(0, 0, 0, 0, 0, 0, 1, 8, C, _stream()) == 1
        assert lib.plx_xent_cls_hp_bwd(0, 0, 0, 0, 0, 0, 1, 8, C, 0.0, _stream()) == 1


def test_one_captured_graph_serves_every_value(cuda):
    """Forward + backward of class_xent(loss_hp=h) captured once: a replay after h.set(...) computes the new values'
    loss, NLL and gradient -- bit for bit the eager ones -- with no re-capture."""
    from polyaxon_amd.ops.lm import class_xent
    from polyaxon_amd.ops.loss_hp import LossHParams

    shape = (8, 264, 257)
    c = _case("cls", shape)
    logits = c["logits"].clone().requires_grad_()
    labels = c["targets"]
    h = LossHParams(cuda)

    def step():
        loss = class_xent(logits, labels, loss_hp=h, n_classes=shape[2])
        (grad,) = torch.autograd.grad(loss * DLOSS, logits)
        return loss.detach(), grad, h.nll.clone()

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    replays = []
    for hp in ({"label_smoothing": 0.0, "z_loss": 0.0}, {"label_smoothing": 0.2, "z_loss": 1e-3}):
        h.set(**hp)
        graph.replay()
        got = [t.clone() for t in static]
        want = step()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a.float(), b.float()) and bool(torch.isfinite(a).all())
        replays.append(got)
    (l0, g0, n0), (l1, g1, n1) = replays
    assert float(l1) != float(l0) and not torch.equal(g0, g1)
    assert torch.equal(n0, n1) and torch.equal(n0, l0)  # the plain NLL does not move with the hyper-parameters


def _trial(ex, seed, steps, **hp):
    ex.reset(seed=seed)
    ex.set_hparams(lr=0.05, momentum=0.9, weight_decay=0.0, **hp)
    out = []
    for _ in range(steps):
        ex.run(1)
        out.append(ex.flat.params.clone())
    torch.cuda.synchronize()
    return out


def test_executor_searches_the_loss_in_one_captured_step(cuda):
    from polyaxon_amd.polyflow.programs import build_program

    plain = build_program("mlp", {"batch": 64}, cuda)
    prog = build_program("mlp", {"batch": 64, "loss_hparams": True}, cuda)
    assert prog.hp_keys == plain.hp_keys + ("label_smoothing", "z_loss")
    plain.warm()
    prog.warm()
    ex0, ex = plain.executor, prog.executor
    assert ex0.graph is not None and ex.graph is not None and ex0.loss_hp is None
    graph = ex.graph
    p0 = _trial(ex0, 3, 3, label_smoothing=0.2, z_loss=0.1)  # no flag: the keys are dropped
    p = _trial(ex, 3, 3, label_smoothing=0.0, z_loss=0.0)
    assert torch.equal(p[2], p0[2])                          # at 0 / 0 the captured step is the plain one, bit for bit
    first = float(ex.losses()[0])
    assert first == float(ex0.losses()[0])
    q = _trial(ex, 3, 1, label_smoothing=0.2)
    assert ex.graph is graph                                 # the same captured step
    assert float(ex.losses()[0]) == first                    # the ring holds the plain NLL: same weights, same batch
    assert not torch.equal(q[0], p[0])                       # and the update came from the smoothed loss
    assert float(ex.train_loss()) != first
    # once the fixed batch is fitted the target's logit stands above the mean logit: smoothing then costs loss
    ex.run(40)
    assert float(ex.train_loss()) > float(ex.losses()[-1])


def test_resnet_tiny_runs_the_fused_pair(cuda, monkeypatch):
    """Eager, bf16 autocast: the classification head's loss is the fused _hp pair, not the torch fallback."""
    from polyaxon_amd.ops import lm
    from polyaxon_amd.polyflow.programs import build_program

    def no_fallback(*a, **k):
        raise AssertionError("the torch fallback ran")

    calls = []
    lib = _native.lib("plx_lm")
    fwd, bwd = lib.plx_xent_cls_hp_fwd, lib.plx_xent_cls_hp_bwd
    monkeypatch.setattr(lm, "_xent_hp_reference", no_fallback)
    monkeypatch.setattr(lib, "plx_xent_cls_hp_fwd", lambda *a: (calls.append("fwd"), fwd(*a))[1])
    monkeypatch.setattr(lib, "plx_xent_cls_hp_bwd", lambda *a: (calls.append("bwd"), bwd(*a))[1])
    prog = build_program("resnet_tiny", {"loss_hparams": True}, cuda)
    ex = prog.executor
    ex.loss_hp.nll.fill_(-1.0)
    ex.reset(seed=1)
    ex.set_hparams(lr=0.01, momentum=0.9, weight_decay=1e-4, label_smoothing=0.2, z_loss=1e-4)
    ex.run(2)
    torch.cuda.synchronize()
    assert calls == ["fwd", "bwd"] * 2
    nll = float(ex.loss_hp.nll)
    assert nll > 0.0 and nll == float(ex.losses()[-1]) and float(ex.train_loss()) != nll
