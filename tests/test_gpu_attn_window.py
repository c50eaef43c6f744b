"""Sliding-window flash attention against an fp64 masked softmax with the band ``i - W < j <= i`` and the bounds of
tests/test_attention_bounds.py (dropout: tests/test_gpu_attn_dropout.py).  Checked once on the CPU: for every (case, W)
the fp64 ``out`` of band W + 1 and of W - 1 exceeds the bound against band W (the seed offset covers S = 65, W = 64)."""
import collections
import ctypes
import zlib

import numpy as np
import pytest
import torch

from polyaxon_amd.ops import attn_dropout as ad
from polyaxon_amd.ops.attn_window import AttnWindowState

U, SCALE, GUARD = 2.0 ** -8, 0.5, 0x7B7B
SEED, KEY, STEP, LAYER, T = 0x0F0F1E1E1234ABCD, (0x1234ABCD, 0x0F0F1E1E), 3, 1, 26
# (B, H, Hkv, S, D): windows.  Wave 32 rows, key tile 64, block 256; S = 600: j0 of q0 = 512 moves between W = 193 / 194
WINDOWS = {(1, 2, 2, 1, 64): [1], (1, 4, 2, 65, 128): [1, 32, 33, 64], (1, 2, 2, 300, 64): [1, 33, 64, 100, 257],
           (1, 4, 1, 600, 128): [1, 40, 64, 193, 194, 300], (3, 6, 2, 70, 64): [7]}
S65, S300, S600 = list(WINDOWS)[1:4]


def _inputs(case):
    B, H, Hkv, S, D = case
    gen = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) + 29)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)  # noqa: E731
    return rnd(B, H, S, D), rnd(B, Hkv, S, D), rnd(B, Hkv, S, D), rnd(B, S, H, D)


def _oracle(case, W, drop=False):
    B, H, Hkv, S, D = case
    q, k, v, g = _inputs(case)
    G = H // Hkv
    Q, dO = q.double(), g.double().transpose(1, 2)
    K, V = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    red = lambda x: x.view(B, Hkv, G, S, D).sum(2)  # noqa: E731
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    P = ((Q @ K.transpose(-1, -2)) * SCALE).masked_fill((j > i) | (j <= i - W), float("-inf")).softmax(-1)
    Mc = 1.0
    if drop:  # the twin's mask, scaled
        m = np.stack([ad.mask_reference(KEY, STEP, LAYER, bh, S, S, T) for bh in range(B * H)])
        Mc = torch.from_numpy(m).view(B, H, S, S).double() * ad.scale(T)
    PM = Mc * P
    O = PM @ V
    bO = U * (PM @ V.abs() + O.abs())
    dS = P * (Mc * (dO @ V.transpose(-1, -2)) - (dO * O).sum(-1, keepdim=True))
    bdS = U * dS.abs() + P * (dO.abs() * bO).sum(-1, keepdim=True)
    dQ, dK, dV = SCALE * (dS @ K), red(SCALE * (dS.transpose(-1, -2) @ Q)), red(PM.transpose(-1, -2) @ dO)
    ref = dict(out=O.transpose(1, 2), dq=dQ, dk=dK, dv=dV)
    bound = dict(out=bO.transpose(1, 2), dq=SCALE * (bdS @ K.abs()) + U * dQ.abs(),
                 dk=red(SCALE * (bdS.transpose(-1, -2) @ Q.abs())) + U * dK.abs(),
                 dv=red(U * (PM.transpose(-1, -2) @ dO.abs())) + U * dV.abs())
    return ref, bound


def _attend(case, dev, window=None, drop=False):
    """out, lse2, dq, dk, dv of flash_attention on the case's inputs, and all of their bytes as ``bits``."""
    from polyaxon_amd.ops.attention import flash_attention

    if drop:
        drop = ad.AttnDropoutState(dev, torch.full((1,), STEP, dtype=torch.int32, device=dev), seed=SEED), LAYER
        drop[0].set(attn_dropout=T / 256.0)
    q, k, v, g = (t.to(dev) for t in _inputs(case))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    out = flash_attention(q, k, v, causal=True, scale=SCALE, drop=drop or None, window=window)
    lse2 = out.grad_fn.saved_tensors[4]
    out.backward(g)
    got = dict(out=out.detach(), lse2=lse2, dq=q.grad, dk=k.grad, dv=v.grad)
    return dict(got, bits=torch.cat([t.view(torch.uint8).flatten() for t in got.values()]))


@pytest.mark.gpu
@pytest.mark.parametrize("case,W,drop", [(c, w, False) for c, ws in WINDOWS.items() for w in ws] + [(S300, 64, True)])
def test_values_against_fp64_at_the_tile_edges(cuda, case, W, drop):
    got = _attend(case, cuda, AttnWindowState(cuda, W), drop)
    assert bool(torch.isfinite(got["lse2"]).all())
    ref, bound = _oracle(case, W, drop)
    r = {n: float(((got[n].cpu().double() - ref[n]).abs() / bound[n].clamp_min(1e-300)).max()) for n in ref}
    assert all(x <= 1.0 for x in r.values()), r


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("case", [S65, S300, S600])
def test_the_window_is_device_data_and_bitwise_plain_where_it_removes_nothing(cuda, case, drop):
    st, S, got = AttnWindowState(cuda), case[3], collections.defaultdict(list)
    for W in (0, S, S + 1000, 40, 40, 100):   # one state, one set of tensors
        st.set(attn_window=W)
        got[W].append(_attend(case, cuda, st, drop)["bits"])
    plain = _attend(case, cuda, None, drop)["bits"]
    assert all(torch.equal(got[W][0], plain) for W in (0, S, S + 1000))
    assert torch.equal(*got[40]) and not torch.equal(got[40][0], got[100][0])
    for W in (40, 100):                       # a fresh state built at that value
        assert torch.equal(got[W][0], _attend(case, cuda, AttnWindowState(cuda, W), drop)["bits"]), W


@pytest.mark.gpu
def test_validation_launches_nothing(cuda):
    from polyaxon_amd.ops import attention

    lib, D = attention._win_lib(), 64
    q, k, v = (torch.zeros(1, h, s, D, dtype=torch.bfloat16, device=cuda) for h, s in ((4, 40), (2, 40), (2, 80)))
    guard = torch.full((6, 2 * 4 * 80 * D), GUARD, dtype=torch.int16, device=cuda)
    win, stream = AttnWindowState(cuda, 8).win.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream
    for kv, causal, w in ((k, True, None), (k, False, win), (v, True, win)):   # null window, causal = 0, S != Skv
        a = attention._args(q, kv, kv, causal, 0.125)
        a.out, a.dq, a.dk, a.dv, a.lse2, a.delta = (t.data_ptr() for t in guard)
        a.o, a.dout, a.so, a.sdo, a.sdq, a.sdk, a.sdv = a.out, q.data_ptr(), a.sq, a.sq, a.sq, a.sk, a.sk
        assert lib.plx_attn_win_fwd(ctypes.byref(a), w, None, None, 0, D, stream) == 1
        assert lib.plx_attn_win_bwd(ctypes.byref(a), w, None, None, 0, D, guard.data_ptr(), stream) == 1
        if w is not None:
            with pytest.raises(ValueError):
                attention.flash_attention(q, kv, kv, causal=causal, window=AttnWindowState(cuda, 8))
    assert bool((guard == GUARD).all())


@pytest.mark.gpu
def test_executor_searches_the_window_in_one_captured_step(cuda, monkeypatch):
    from polyaxon_amd.ops import attention
    from polyaxon_amd.polyflow.programs import build_program

    params = {"graph": True, "heads": 1}   # heads: 1 gives gpt2_tiny head_dim 64: the HIP kernels
    plain = build_program("gpt2_tiny", params, cuda)
    plain.warm()
    calls = collections.Counter()
    for n in ("plx_attn_fwd", "plx_attn_bwd", "plx_attn_win_fwd"):
        lib = attention._win_lib() if "win" in n else attention._lib()
        monkeypatch.setattr(lib, n, lambda *a, _f=getattr(lib, n), _n=n: calls.update([_n]) or _f(*a))
    prog = build_program("gpt2_tiny", dict(params, attn_window=True), cuda)
    prog.warm()
    assert calls["plx_attn_win_fwd"] > 0 and calls["plx_attn_fwd"] == 0 and calls["plx_attn_bwd"] == 0
    ex0, ex, graph = plain.executor, prog.executor, prog.executor.graph
    assert graph is not None and ex0.graph is not None
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k != "attn_window"}
    c0 = ex0.data.counter.clone()

    def trial(e, W):
        e.data.counter.copy_(c0)
        e.reset(seed=3)
        e.set_hparams(**base, attn_window=W)   # the plain executor drops the key
        e.run(3)
        return e.flat.params.clone()

    p0, p8 = trial(ex0, 8), trial(ex, 8)
    assert not torch.equal(p8, p0) and bool(torch.isfinite(p8).all())
    assert torch.equal(trial(ex, 0), p0)               # no window: bitwise the plain program
    assert torch.equal(trial(ex, 8), p8) and ex.graph is graph   # the same captured step
    ex.model.set_attn_window(None)
    n = calls["plx_attn_win_fwd"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ex.model(ex.x)
    assert calls["plx_attn_fwd"] == 2 and calls["plx_attn_win_fwd"] == n
