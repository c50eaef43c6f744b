"""Document-masked flash attention against an fp64 masked softmax with the mask ``start[i] <= j <= i`` and the
a-priori bounds of tests/test_gpu_attn_window.py (dropout: the host twin's mask).  Checked once on the CPU: for every
case and every document boundary, the fp64 ``out`` with that boundary moved by +1 and by -1 exceeds the bound against
the unmoved one, so an off-by-one in the kernels cannot pass -- with one exception: in the case of 300 one-position
documents the boundary at 143 gives 0.06 of the bound (query 143 puts almost no weight on key 142); the 298 other
boundaries of that case exceed it."""
import collections
import ctypes
import zlib

import pytest
import torch

from polyaxon_amd.ops import attn_dropout as ad
from polyaxon_amd.ops.attn_doc import AttnDocState

U, SCALE, GUARD = 2.0 ** -8, 0.5, 0x7B7B
SEED, KEY, STEP, LAYER, T = 0x0F0F1E1E1234ABCD, (0x1234ABCD, 0x0F0F1E1E), 3, 1, 26
S300 = (1, 2, 2, 300, 64)
# (B, H, Hkv, S, D), the document starts of every batch row, dropout.  Wave 32 rows, key tile 64, block 256
CASES = [((1, 2, 2, 1, 64), [[0]], False)]
CASES += [((1, 4, 2, 65, 128), [s], False) for s in ([0, 1], [0, 32], [0, 33], [0, 64])]
CASES += [(S300, [s], False) for s in ([0, 33, 64, 100, 257], [0, 255, 256], list(range(300)))]
CASES += [((1, 4, 1, 600, 128), [[0, 40, 64, 193, 512, 513]], False),
          ((3, 6, 2, 70, 64), [[0], [0, 7], [0, 64, 69]], False), (S300, [[0, 64, 257]], True)]


def _tables(starts, S):  # start / end [B, S] int32 of the documents that open at starts[b]
    pos = torch.arange(S)
    opens = [torch.tensor(s + [S]) for s in starts]
    start = torch.stack([o[torch.searchsorted(o, pos, right=True) - 1] for o in opens])
    end = torch.stack([o[torch.searchsorted(o, pos, right=True)] for o in opens])
    return start.int(), end.int()


def _inputs(case):
    B, H, Hkv, S, D = case
    gen = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) + 29)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)  # noqa: E731
    return rnd(B, H, S, D), rnd(B, Hkv, S, D), rnd(B, Hkv, S, D), rnd(B, S, H, D)


def _oracle(case, starts, drop=False):
    import numpy as np

    B, H, Hkv, S, D = case
    q, k, v, g = _inputs(case)
    G = H // Hkv
    Q, dO = q.double(), g.double().transpose(1, 2)
    K, V = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    red = lambda x: x.view(B, Hkv, G, S, D).sum(2)  # noqa: E731
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    hidden = (j > i) | (j < _tables(starts, S)[0][:, None, :, None])
    P = ((Q @ K.transpose(-1, -2)) * SCALE).masked_fill(hidden, float("-inf")).softmax(-1)
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


def _attend(case, dev, doc=None, drop=False):
    """out, lse2, dq, dk, dv of flash_attention on the case's inputs, and all of their bytes as ``bits``."""
    from polyaxon_amd.ops.attention import flash_attention

    if drop:
        drop = ad.AttnDropoutState(dev, torch.full((1,), STEP, dtype=torch.int32, device=dev), seed=SEED), LAYER
        drop[0].set(attn_dropout=T / 256.0)
    q, k, v, g = (t.to(dev) for t in _inputs(case))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    out = flash_attention(q, k, v, causal=True, scale=SCALE, drop=drop or None, doc=doc)
    lse2 = out.grad_fn.saved_tensors[4]
    out.backward(g)
    got = dict(out=out.detach(), lse2=lse2, dq=q.grad, dk=k.grad, dv=v.grad)
    return dict(got, bits=torch.cat([t.view(torch.uint8).flatten() for t in got.values()]))


@pytest.mark.gpu
@pytest.mark.parametrize("case,starts,drop", CASES, ids=lambda x: None if isinstance(x, bool) else str(x)[:32])
def test_values_against_fp64_at_the_tile_edges(cuda, case, starts, drop):
    st = AttnDocState(cuda, case[0], case[3], 0)
    st.set_tables(*_tables(starts, case[3]))
    got = _attend(case, cuda, st, drop)
    assert bool(torch.isfinite(got["lse2"]).all())
    ref, bound = _oracle(case, starts, drop)
    r = {n: float(((got[n].cpu().double() - ref[n]).abs() / bound[n].clamp_min(1e-300)).max()) for n in ref}
    assert all(x <= 1.0 for x in r.values()), r


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [False, True])
def test_the_tables_are_device_data_and_bitwise_plain_with_one_document(cuda, drop):
    st, got = AttnDocState(cuda, 1, 300, 0), []   # one state, one set of tensors
    assert torch.equal(_attend(S300, cuda, st, drop)["bits"], _attend(S300, cuda, None, drop)["bits"])
    for starts in ([0, 100], [0, 64, 257], [0, 100]):
        st.set_tables(*_tables([starts], 300))
        got.append(_attend(S300, cuda, st, drop)["bits"])
    assert not torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


@pytest.mark.gpu
def test_validation_launches_nothing(cuda):
    from polyaxon_amd.ops import attention

    lib, D = attention._doc_lib(), 64
    q, k, v = (torch.zeros(1, h, s, D, dtype=torch.bfloat16, device=cuda) for h, s in ((4, 40), (2, 40), (2, 80)))
    guard = torch.full((6, 2 * 4 * 80 * D), GUARD, dtype=torch.int16, device=cuda)
    tab, stream = AttnDocState(cuda, 1, 40, 0), torch.cuda.current_stream(cuda).cuda_stream
    s, e = tab.start.data_ptr(), tab.end.data_ptr()
    # a null table (either), causal = 0, S != Skv
    for kv, causal, ts, te in ((k, True, None, e), (k, True, s, None), (k, False, s, e), (v, True, s, e)):
        a = attention._args(q, kv, kv, causal, 0.125)
        a.out, a.dq, a.dk, a.dv, a.lse2, a.delta = (t.data_ptr() for t in guard)
        a.o, a.dout, a.so, a.sdo, a.sdq, a.sdk, a.sdv = a.out, q.data_ptr(), a.sq, a.sq, a.sq, a.sk, a.sk
        assert lib.plx_attn_doc_fwd(ctypes.byref(a), ts, te, None, None, 0, D, stream) == 1
        assert lib.plx_attn_doc_bwd(ctypes.byref(a), ts, te, None, None, 0, D, guard.data_ptr(), stream) == 1
    assert bool((guard == GUARD).all())


@pytest.mark.gpu
def test_one_captured_step_follows_the_batch(cuda, monkeypatch):
    from polyaxon_amd.ops import attention
    from polyaxon_amd.polyflow.programs import build_program

    # heads: 1 gives gpt2_tiny head_dim 64: the HIP kernels; 4 active tokens: every batch holds EOS = 1, never 200
    params = {"graph": True, "heads": 1, "active_vocab": 4}
    plain = build_program("gpt2_tiny", params, cuda)
    plain.warm()
    calls = collections.Counter()
    for n, lib in (("plx_attn_fwd", attention._lib()), ("plx_attn_doc_fwd", attention._doc_lib())):
        monkeypatch.setattr(lib, n, lambda *a, _f=getattr(lib, n), _n=n: calls.update([_n]) or _f(*a))
    progs = {eos: build_program("gpt2_tiny", dict(params, attn_doc_eos=eos), cuda) for eos in (1, 200)}
    for p in progs.values():
        p.warm()
    assert calls["plx_attn_doc_fwd"] > 0 and calls["plx_attn_fwd"] == 0
    c0 = plain.executor.data.counter.clone()

    def trial(e, steps):
        e.data.counter.copy_(c0)
        e.reset(seed=3)
        e.set_hparams(**plain.info["warm_hparams"])
        e.run(steps)   # a fresh batch every replay
        return e.flat.params.clone(), e.attn_doc.start.clone() if e.attn_doc else None

    ex, graph = progs[1].executor, progs[1].executor.graph
    (p1, s1), (p2, s2) = trial(ex, 1), trial(ex, 2)
    row = ex.x[0].tolist()   # the tables of the last replay's own batch, by the definition
    assert s2[0].tolist() == [max(t for t in range(i + 1) if t == 0 or row[t - 1] == 1) for i in range(len(row))]
    assert not torch.equal(s1, s2) and graph is not None and ex.graph is graph   # two batches, one captured step
    assert bool(torch.isfinite(p2).all()) and not torch.equal(p2, trial(plain.executor, 2)[0])
    assert torch.equal(trial(progs[200].executor, 2)[0], trial(plain.executor, 2)[0])   # no EOS: bitwise plain
