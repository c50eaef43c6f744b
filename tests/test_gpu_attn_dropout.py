"""Attention dropout inside the flash-attention kernels (csrc/attn_kernels.hip ``plx_attn_drop_fwd`` / ``_bwd``).

Layout of this file:

1. the fp64 oracle with the host twin's mask and its per-element bounds, an fp32 emulation of the DROP dataflow (CPU
   tests: the emulation is inside the bound, injected defects are outside);
2. exact read-outs of the mask each kernel draws, bit for bit against the twin;
3. values of out, dq, dk, dv against the bounds, lse2, bitwise equality with the plain kernels at T = 0, determinism;
4. direct ctypes calls: guard patterns around every output, argument validation;
5. one captured gpt2_tiny step through the executor, and the feature-off path.

Bounds.  With M the 0/1 mask, c the fp32 scale and P the softmax probabilities (fp64), the kernels round to bf16 at
these points and nowhere else; fp32 accumulation, v_exp_f32 and the fp32 products with c are left out (below 2 % of u)
as in tests/test_attention_bounds.py, whose derivation this one follows term by term:

* forward: the operand M o p of O^T += V^T (M o p)^T is rounded (acc_frag), the row sum keeps the unrounded,
  undropped p, and the finished row o * (c / l) is rounded once:           b_out = u ((cM o P) |V| + |O|);
* delta = rowsum(dO o O) reads the stored bf16 O:                          b_delta = rowsum(|dO| b_out);
* dS = p (c M dP - delta) is rounded as the MFMA operand in the dQ and the dK/dV kernel; c M dP itself stays fp32:
                                                                           b_dS = u |dS| + P b_delta;
* dQ = scale dS K, its row rounded once:                                   b_dQ = scale b_dS |K| + u |dQ|;
* dK = scale dS^T Q summed over the GQA group, rounded once:               b_dK = scale b_dS^T |Q| + u |dK|;
* dV = c (M o p)^T dO, the operand M o p rounded, the finished row (times c) rounded once:
                                                                           b_dV = u (cM o P)^T |dO| + u |dV|.

The statistic is max |got - ref| / bound and the assertion is <= 1.0.
"""
import ctypes
import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

from polyaxon_amd.ops import attn_dropout as ad

U = 2.0 ** -8
LOG2E = 1.4426950408889634
GUARD16, GUARD32 = 0x7B7B, 0x7B7B7B7B
SEED = 0x0F0F1E1E1234ABCD            # key words (0x1234ABCD, 0x0F0F1E1E): the keys tests/test_attn_dropout.py checks
KEY = (0x1234ABCD, 0x0F0F1E1E)
STEP, LAYER = 3, 1
RATES = [0, 26, 128, 255]

Case = namedtuple("Case", "B H Hkv S Skv D causal")

# Tile facts: a wave owns 32 rows, a key tile is 64, a forward / dQ / dK-dV block is 256.  S = Skv on both sides of
# each edge, S != Skv in each direction; D, the mask and the head grouping alternate; B * H = 6 is no power of two.
CASES = [Case(1, 2, 2, 1, 1, 64, True), Case(1, 8, 1, 33, 33, 128, False), Case(3, 2, 2, 65, 65, 64, True),
         Case(1, 4, 2, 129, 129, 128, True), Case(1, 2, 2, 257, 257, 64, False), Case(1, 4, 2, 257, 257, 128, True),
         Case(1, 4, 2, 70, 200, 64, False), Case(1, 8, 1, 200, 70, 128, True)]


def _id(c) -> str:
    if not isinstance(c, Case):
        return str(c)
    return f"{c.B}x{c.H}x{c.Hkv}-S{c.S}-Skv{c.Skv}-D{c.D}-{'causal' if c.causal else 'full'}"


def _visible(S, Skv, causal):
    vis = torch.ones(S, Skv, dtype=torch.bool)
    return vis.tril() if causal else vis


@functools.lru_cache(maxsize=None)
def _keep(c: Case, T: int, step: int = STEP, layer: int = LAYER):
    """bool [B, H, S, Skv]: the twin's mask of every (batch, head) of a case."""
    m = np.stack([ad.mask_reference(KEY, step, layer, bh, c.S, c.Skv, T) for bh in range(c.B * c.H)])
    return torch.from_numpy(m).view(c.B, c.H, c.S, c.Skv)


def _inputs(c: Case):
    gen = torch.Generator().manual_seed(zlib.crc32(_id(c).encode()))
    rnd = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)  # noqa: E731
    return rnd(c.B, c.H, c.S, c.D), rnd(c.B, c.Hkv, c.Skv, c.D), rnd(c.B, c.Hkv, c.Skv, c.D), rnd(c.B, c.S, c.H, c.D)


# ---------------------------------------------------------------------------------------------------- 1. the oracle
def _oracle(q, k, v, g, causal, scale, keep, cs):
    """fp64 reference and per-element bounds (module docstring) of out [B,S,H,D], dq, dk, dv, and the lse2."""
    B, H, S, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    G = H // Hkv
    Q, dO = q.double(), g.double().transpose(1, 2)
    K, V = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    red = lambda x: x.view(B, Hkv, G, Skv, D).sum(2)  # noqa: E731
    s = ((Q @ K.transpose(-1, -2)) * scale).masked_fill(~_visible(S, Skv, causal), -math.inf)
    P = s.softmax(-1)
    lse2 = torch.logsumexp(s, -1) * LOG2E
    Mc = keep.double() * cs
    PM = Mc * P
    O = PM @ V
    bO = U * (PM @ V.abs() + O.abs())
    delta = (dO * O).sum(-1, keepdim=True)
    bdelta = (dO.abs() * bO).sum(-1, keepdim=True)
    dS = P * (Mc * (dO @ V.transpose(-1, -2)) - delta)
    bdS = U * dS.abs() + P * bdelta
    dQ = scale * (dS @ K)
    bdQ = scale * (bdS @ K.abs()) + U * dQ.abs()
    dK = red(scale * (dS.transpose(-1, -2) @ Q))
    bdK = red(scale * (bdS.transpose(-1, -2) @ Q.abs())) + U * dK.abs()
    dV = red(PM.transpose(-1, -2) @ dO)
    bdV = red(U * (PM.transpose(-1, -2) @ dO.abs())) + U * dV.abs()
    ref = dict(out=O.transpose(1, 2), dq=dQ, dk=dK, dv=dV)
    bound = dict(out=bO.transpose(1, 2), dq=bdQ, dk=bdK, dv=bdV)
    return ref, bound, lse2


def _ratio(got, ref, bound) -> float:
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


def _ratios(got: dict, data) -> dict:
    return {n: _ratio(got[n].cpu(), data.ref[n], data.bound[n]) for n in ("out", "dq", "dk", "dv")}


Data = namedtuple("Data", "q k v g scale ref bound lse2")


@functools.lru_cache(maxsize=None)
def _data(c: Case, T: int) -> Data:
    """Inputs, fp64 reference and bounds of a case at a rate: computed once, shared read-only."""
    q, k, v, g = _inputs(c)
    scale = 1.0 / math.sqrt(c.D)
    ref, bound, lse2 = _oracle(q, k, v, g, c.causal, scale, _keep(c, T), ad.scale(T))
    return Data(q, k, v, g, scale, ref, bound, lse2)


def _emulate(c: Case, T: int, defect=None):
    """The DROP dataflow in fp32 torch with .to(bfloat16) at exactly the oracle's rounding points.  ``defect``: 'c2'
    (the scale applied twice to the output and to dV), 'step' (the backward draws the mask of step t + 1)."""
    f32 = torch.float32
    bf = lambda x: x.to(torch.bfloat16).to(f32)  # noqa: E731
    d = _data(c, T)
    B, H, Hkv, S, Skv, D = c.B, c.H, c.Hkv, c.S, c.Skv, c.D
    G = H // Hkv
    cs = ad.scale(T)
    M = _keep(c, T).to(f32)
    Mb = _keep(c, T, step=STEP + 1).to(f32) if defect == "step" else M
    Q, dO = d.q.to(f32), d.g.to(f32).transpose(1, 2)
    K, V = d.k.to(f32).repeat_interleave(G, 1), d.v.to(f32).repeat_interleave(G, 1)
    vis = _visible(S, Skv, c.causal)
    sc = ((Q @ K.transpose(-1, -2)) * float(torch.tensor(d.scale * LOG2E, dtype=f32))).masked_fill(~vis, -math.inf)
    m = sc.amax(-1, keepdim=True)
    p = torch.exp2(sc - m)
    l = p.sum(-1, keepdim=True)
    cf = cs * cs if defect == "c2" else cs
    out = bf((bf(M * p) @ V) * (cf / l))
    lse2 = (m + torch.log2(l)).squeeze(-1)
    delta = (dO * out).sum(-1, keepdim=True)
    p = torch.where(vis, torch.exp2(sc - lse2[..., None]), torch.zeros_like(sc))
    dS = bf(p * (Mb * cs * (dO @ V.transpose(-1, -2)) - delta))
    dq = bf((dS @ K) * d.scale)
    red = lambda x: bf(x.view(B, Hkv, G, Skv, D).sum(2))  # noqa: E731
    dk = red((dS.transpose(-1, -2) @ Q) * d.scale)
    dv = red((bf(Mb * p).transpose(-1, -2) @ dO) * cf)
    return dict(out=out.transpose(1, 2), dq=dq, dk=dk, dv=dv), lse2


@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_emulation_stays_inside_the_bound(case, T):
    got, _ = _emulate(case, T)
    r = _ratios(got, _data(case, T))
    print(f"emulation {_id(case)} T={T}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    assert all(x <= 1.0 for x in r.values()), r


@pytest.mark.parametrize("T", [26, 128])
@pytest.mark.parametrize("case", [c for c in CASES if c.S > 1], ids=_id)
def test_injected_defect_exceeds_the_bound(case, T):
    """The scale applied twice shows in out and dv; the backward on the next step's mask shows in dq, dk and dv."""
    d = _data(case, T)
    r = _ratios(_emulate(case, T, "c2")[0], d)
    print(f"c2 {_id(case)} T={T}: " + " ".join(f"{n}={x:.2f}" for n, x in r.items()))
    assert r["out"] > 1.0 and r["dv"] > 1.0, r
    r = _ratios(_emulate(case, T, "step")[0], d)
    print(f"step {_id(case)} T={T}: " + " ".join(f"{n}={x:.2f}" for n, x in r.items()))
    assert r["dq"] > 1.0 and r["dk"] > 1.0 and r["dv"] > 1.0, r


# ------------------------------------------------------------------------------------------------ GPU helpers
def _state(dev, T, step=STEP):
    st = ad.AttnDropoutState(dev, torch.full((1,), step, dtype=torch.int32, device=dev), seed=SEED)
    st.set(attn_dropout=T / 256.0)
    assert st.T == T and st.key == KEY
    return st


class _Waves:
    """The forward and dQ kernels at ``n`` waves per workgroup inside the block, 8 (the default) restored after it."""

    def __init__(self, n):
        from polyaxon_amd.ops import attention

        self.lib, self.n = attention._lib(), n

    def _set(self, n):
        self.lib.plx_attn_set_fwd_waves(n)
        self.lib.plx_attn_set_dq_waves(n)

    def __enter__(self):
        self._set(self.n)
        return self.lib

    def __exit__(self, *exc):
        self._set(8)


def _attend(q, k, v, g, causal, st, layer=LAYER, backward=True):
    """out, lse2 (and dq, dk, dv) of flash_attention on device tensors; ``st`` None: the plain kernels."""
    from polyaxon_amd.ops.attention import flash_attention

    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = flash_attention(q, k, v, causal=causal, drop=None if st is None else (st, layer))
    got = dict(out=out.detach(), lse2=out.grad_fn.saved_tensors[4])
    if backward:
        out.backward(g)
        got.update(dq=q.grad, dk=k.grad, dv=v.grad)
    return got


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _windows(n, D):
    return range(0, n, D)


# ------------------------------------------------------------------------------------- 2. exact mask read-outs
# With Q = 0 (or K = 0) every score is 0 and P is uniform over the visible keys, 1 / nvis, whatever the other operand
# is.  A one-hot operand then copies single elements of the masked tile into an output, D keys or queries at a time.
def _expect(c: Case, T: int):
    return _keep(c, T) & _visible(c.S, c.Skv, c.causal)


def _forward_readout(c: Case, T: int, dev):
    """bool [B, H, S, Skv]: where the forward kernel kept a probability.  V rows one-hot inside a window of D keys."""
    st = _state(dev, T)
    q = torch.zeros(c.B, c.H, c.S, c.D, dtype=torch.bfloat16, device=dev)
    k = _inputs(c)[1].to(dev)
    got = torch.zeros(c.B, c.H, c.S, c.Skv, dtype=torch.bool)
    for w0 in _windows(c.Skv, c.D):
        n = min(c.D, c.Skv - w0)
        v = torch.zeros(c.B, c.Hkv, c.Skv, c.D, dtype=torch.bfloat16, device=dev)
        v[:, :, w0:w0 + n, :n] = torch.eye(n, dtype=torch.bfloat16, device=dev)
        out = _attend(q, k, v, None, c.causal, st, backward=False)["out"]        # [B, S, H, D]
        got[..., w0:w0 + n] = (out[..., :n] != 0).transpose(1, 2).cpu()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_mask_is_the_twin(cuda, case, T):
    want = _expect(case, T)
    assert torch.equal(_forward_readout(case, T, cuda), want)
    with _Waves(4):
        assert torch.equal(_forward_readout(case, T, cuda), want)    # the mask does not depend on the block size


def _sign_rows(c: Case, T: int):
    """Rows whose dS sign reads the mask: 0 < delta < c, i.e. some but not all visible keys kept.  delta is the
    stored bf16 c * kept / nvis: with >= 1 key of <= 257 dropped it is below c by >= c / 257 > 2^-8 c."""
    kept = _expect(c, T).sum(-1)
    nvis = _visible(c.S, c.Skv, c.causal).sum(-1)
    return (kept > 0) & (kept < nvis)          # [B, H, S]


def _dq_readout(c: Case, T: int, dev):
    """sign of dS^T as the dQ kernel forms it: dO = e_0 and V[:, 0] = 1 give dP = 1, K one-hot inside a window copies
    dS[q, w0 + j] = P (c M - delta_q) into dQ[q, j]."""
    st = _state(dev, T)
    q = torch.zeros(c.B, c.H, c.S, c.D, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(c.B, c.Hkv, c.Skv, c.D, dtype=torch.bfloat16, device=dev)
    v[..., 0] = 1
    g = torch.zeros(c.B, c.S, c.H, c.D, dtype=torch.bfloat16, device=dev)
    g[..., 0] = 1
    got = torch.zeros(c.B, c.H, c.S, c.Skv)
    for w0 in _windows(c.Skv, c.D):
        n = min(c.D, c.Skv - w0)
        k = torch.zeros(c.B, c.Hkv, c.Skv, c.D, dtype=torch.bfloat16, device=dev)
        k[:, :, w0:w0 + n, :n] = torch.eye(n, dtype=torch.bfloat16, device=dev)
        got[..., w0:w0 + n] = _attend(q, k, v, g, c.causal, st)["dq"][..., :n].float().cpu()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("T", RATES[1:])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dq_mask_is_the_twin(cuda, case, T):
    want, rows = _expect(case, T), _sign_rows(case, T)
    vis = _visible(case.S, case.Skv, case.causal).expand_as(want)
    for waves in (8, 4):
        with _Waves(waves):
            ds = _dq_readout(case, T, cuda)
        assert torch.equal((ds > 0)[rows], want[rows]), waves
        assert torch.equal((ds < 0)[rows], (vis & ~want)[rows]), waves
        assert float(ds[~vis].abs().max()) == 0.0 if bool((~vis).any()) else True


def _dkdv_readout(c: Case, T: int, dev):
    """The dK/dV kernel's two uses of the mask, one query head of each GQA group at a time (dK and dV sum the group):
    dV with dO one-hot per query of a window reads M o P; dK with K = 0, Q one-hot per query of a window, dO = e_0 and
    V[:, 0] = 1 reads the sign of dS."""
    st = _state(dev, T)
    G = c.H // c.Hkv
    zeros = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)  # noqa: E731
    kept = torch.zeros(c.B, c.H, c.S, c.Skv, dtype=torch.bool)
    ds = torch.zeros(c.B, c.H, c.S, c.Skv)
    k_rand = _inputs(c)[1].to(dev)
    v1 = zeros(c.B, c.Hkv, c.Skv, c.D)
    v1[..., 0] = 1
    g1 = zeros(c.B, c.S, c.H, c.D)
    g1[..., 0] = 1
    for hg in range(G):
        heads = list(range(hg, c.H, G))          # head hg of every group
        for w0 in _windows(c.S, c.D):
            n = min(c.D, c.S - w0)
            eye = torch.eye(n, dtype=torch.bfloat16, device=dev)
            g = zeros(c.B, c.S, c.H, c.D)
            g[:, w0:w0 + n, heads, :n] = eye[None, :, None, :]
            dv = _attend(zeros(c.B, c.H, c.S, c.D), k_rand, v1, g, c.causal, st)["dv"]      # [B, Hkv, Skv, D]
            kept[:, heads, w0:w0 + n] = (dv[..., :n] != 0).transpose(-1, -2).cpu()
            q = zeros(c.B, c.H, c.S, c.D)
            q[:, heads, w0:w0 + n, :n] = eye
            dk = _attend(q, zeros(c.B, c.Hkv, c.Skv, c.D), v1, g1, c.causal, st)["dk"]
            ds[:, heads, w0:w0 + n] = dk[..., :n].float().transpose(-1, -2).cpu()
    return kept, ds


@pytest.mark.gpu
@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dkdv_masks_are_the_twin(cuda, case, T):
    want, rows = _expect(case, T), _sign_rows(case, T)
    vis = _visible(case.S, case.Skv, case.causal).expand_as(want)
    kept, ds = _dkdv_readout(case, T, cuda)
    assert torch.equal(kept, want)
    assert torch.equal((ds > 0)[rows], want[rows])
    assert torch.equal((ds < 0)[rows], (vis & ~want)[rows])


# --------------------------------------------------------------------------------------------------- 3. values
def _run(c: Case, T, dev, step=STEP, plain=False):
    d = _data(c, T if T is not None else 0)
    st = None if plain else _state(dev, T, step)
    return _attend(d.q.to(dev), d.k.to(dev), d.v.to(dev), d.g.to(dev), c.causal, st)


@pytest.mark.gpu
@pytest.mark.parametrize("T", RATES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_values_within_the_bound_and_lse2_untouched(cuda, case, T):
    d = _data(case, T)
    for waves in (8, 4):
        with _Waves(waves):
            got = _run(case, T, cuda)
            lse2 = _run(case, 0, cuda, plain=True)["lse2"]
        r = _ratios(got, d)
        print(f"kernel {_id(case)} T={T} waves={waves}: " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
        assert _same(got["lse2"], lse2), waves          # the statistics use the undropped probabilities
        for name, x in r.items():
            assert x <= 1.0, (waves, name, r)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bitwise_the_plain_kernels_at_zero(cuda, case):
    for waves in (8, 4):
        with _Waves(waves):
            plain, zero = _run(case, 0, cuda, plain=True), _run(case, 0, cuda)
        for name in ("out", "lse2", "dq", "dk", "dv"):
            assert _same(zero[name], plain[name]), (waves, name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[3], CASES[4], CASES[7]], ids=_id)
def test_deterministic_and_a_new_step_is_a_new_mask(cuda, case):
    one, two, other = _run(case, 128, cuda), _run(case, 128, cuda), _run(case, 128, cuda, step=STEP + 1)
    for name in ("out", "lse2", "dq", "dk", "dv"):
        assert _same(one[name], two[name]), name
    assert _same(one["lse2"], other["lse2"])
    for name in ("out", "dq", "dk", "dv"):
        assert not _same(one[name], other[name]), name


# ------------------------------------------------------------------------------------------- 4. direct ctypes calls
def _guarded(dev, sizes, strides, pad=64):
    extent = 1 + sum((n - 1) * s for n, s in zip(sizes, strides))
    buf = torch.full((pad + extent + pad,), GUARD16, dtype=torch.int16, device=dev)
    return buf, buf.view(torch.bfloat16).as_strided(sizes, strides, pad)


def _guarded_f32(dev, n, pad=64):
    buf = torch.full((pad + n + pad,), GUARD32, dtype=torch.int32, device=dev)
    return buf, buf.view(torch.float32)[pad:pad + n]


def _untouched(buf, view) -> bool:
    pat = GUARD16 if buf.dtype == torch.int16 else GUARD32
    view.view(buf.dtype).fill_(pat)
    return bool((buf == pat).all())


def _st(view):
    from polyaxon_amd.ops.attention import _Strides

    return _Strides(view.stride(0), view.stride(1), view.stride(2))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[2], CASES[6], CASES[7]], ids=_id)
def test_direct_strided_call_keeps_its_guards(cuda, case):
    """plx_attn_drop_fwd / _bwd on padded, non-dense output strides inside guard-filled buffers: nothing outside the
    S / Skv rows is written and the results are those of the wrapper's dense call, bit for bit."""
    from polyaxon_amd.ops import attention
    from polyaxon_amd.ops.attention import _AttnArgs, _zero_page

    T = 26
    c, d, dev = case, _data(case, T), cuda
    B, H, Hkv, S, Skv, D = c.B, c.H, c.Hkv, c.S, c.Skv, c.D
    lib, st, e = attention._lib(), _state(dev, T), 8
    q, k, v = d.q.to(dev), d.k.to(dev), d.v.to(dev)
    g = d.g.to(dev).transpose(1, 2)
    rs = H * (D + e) + e
    obuf, out = _guarded(dev, (B, H, S, D), (S * rs + 3 * e, D + e, rs, 1))
    hm = lambda nh, rows: ((nh * (rows * (D + e) + e) + 2 * e), rows * (D + e) + e, D + e, 1)  # noqa: E731
    qbuf, dq = _guarded(dev, (B, H, S, D), hm(H, S))
    kbuf, dk = _guarded(dev, (B, Hkv, Skv, D), hm(Hkv, Skv))
    vbuf, dv = _guarded(dev, (B, Hkv, Skv, D), hm(Hkv, Skv))
    lbuf, lse2 = _guarded_f32(dev, B * H * S)
    dbuf, delta = _guarded_f32(dev, B * H * S)
    nws = int(lib.plx_attn_bwd_workspace(B, H, Hkv, Skv, D)) // 4
    wbuf, ws = _guarded_f32(dev, max(nws, 1))
    a = _AttnArgs()
    a.q, a.k, a.v, a.sq, a.sk, a.sv = q.data_ptr(), k.data_ptr(), v.data_ptr(), _st(q), _st(k), _st(v)
    a.B, a.H, a.Hkv, a.S, a.Skv, a.causal = B, H, Hkv, S, Skv, int(c.causal)
    a.scale, a.c = d.scale, d.scale * LOG2E
    a.zero = _zero_page(dev).data_ptr()
    a.out, a.so, a.lse2 = out.data_ptr(), _st(out), lse2.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    hp, step = st.hp.data_ptr(), st.step_counter.data_ptr()
    assert lib.plx_attn_drop_fwd(ctypes.byref(a), hp, step, LAYER, D, stream) == 0
    a.o, a.dout, a.sdo, a.delta = out.data_ptr(), g.data_ptr(), _st(g), delta.data_ptr()
    a.dq, a.dk, a.dv, a.sdq, a.sdk, a.sdv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _st(dq), _st(dk), _st(dv)
    assert lib.plx_attn_drop_bwd(ctypes.byref(a), hp, step, LAYER, D, ws.data_ptr() if nws else None, stream) == 0
    torch.cuda.synchronize(dev)
    got = dict(out=out.transpose(1, 2).clone(), dq=dq.clone(), dk=dk.clone(), dv=dv.clone(),
               lse2=lse2.view(B, H, S).clone())
    pairs = [(obuf, out), (qbuf, dq), (kbuf, dk), (vbuf, dv), (lbuf, lse2), (dbuf, delta), (wbuf, ws)]
    names = ["out", "dq", "dk", "dv", "lse2", "delta", "workspace"]
    touched = [nm for nm, (b, vw) in zip(names, pairs) if not _untouched(b, vw)]
    assert not touched, touched
    want = _run(c, T, dev)
    for name in ("out", "lse2", "dq", "dk", "dv"):
        assert _same(got[name], want[name]), name


@pytest.mark.gpu
def test_argument_validation_launches_nothing(cuda):
    from polyaxon_amd.ops import attention
    from polyaxon_amd.ops.attention import _AttnArgs, _Strides

    lib = attention._lib()
    B, H, Hkv, S, D = 1, 4, 2, 40, 64
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=cuda)  # noqa: E731
    q, k, v, g = bf(B, H, S, 128), bf(B, Hkv, S, 128), bf(B, Hkv, S, 128), bf(B, H, S, 128)
    outs = [torch.full((B * H * S * 128,), GUARD16, dtype=torch.int16, device=cuda) for _ in range(4)]
    f32s = [torch.full((B * H * S,), GUARD32, dtype=torch.int32, device=cuda) for _ in range(2)]
    ws = torch.zeros(2 * B * H * S * 128, dtype=torch.float32, device=cuda)
    dense = lambda nh, d: _Strides(nh * S * d, S * d, d)  # noqa: E731
    st = _state(cuda, 26)
    hp, step = st.hp.data_ptr(), st.step_counter.data_ptr()

    def args(d=D, **over):
        a = _AttnArgs()
        a.q, a.k, a.v, a.dout = q.data_ptr(), k.data_ptr(), v.data_ptr(), g.data_ptr()
        a.out, a.dq, a.dk, a.dv = (t.data_ptr() for t in outs)
        a.o, a.lse2, a.delta = outs[0].data_ptr(), f32s[0].data_ptr(), f32s[1].data_ptr()
        a.sq = a.so = a.sdo = a.sdq = dense(H, d)
        a.sk = a.sv = a.sdk = a.sdv = dense(Hkv, d)
        a.B, a.H, a.Hkv, a.S, a.Skv, a.causal = B, H, Hkv, S, S, 1
        a.scale, a.c = 0.125, 0.125 * LOG2E
        a.zero = attention._zero_page(cuda).data_ptr()
        for name, val in over.items():
            setattr(a, name, val)
        return a

    stream = torch.cuda.current_stream(cuda).cuda_stream
    fwd = lambda a, h=hp, t=step, l=LAYER, d=D: lib.plx_attn_drop_fwd(ctypes.byref(a), h, t, l, d, stream)  # noqa: E731
    bwd = lambda a, h=hp, t=step, l=LAYER, d=D, w=ws.data_ptr(): lib.plx_attn_drop_bwd(  # noqa: E731
        ctypes.byref(a), h, t, l, d, w, stream)
    assert fwd(args(), h=None) == 1 and bwd(args(), h=None) == 1
    assert fwd(args(), t=None) == 1 and bwd(args(), t=None) == 1
    assert fwd(args(), l=32768) == 1 and bwd(args(), l=32768) == 1
    assert fwd(args(), l=-1) == 1 and bwd(args(), l=-1) == 1
    assert fwd(args(B=16384)) == 1 and bwd(args(B=16384)) == 1              # B * H = 65536
    assert fwd(args(96), d=96) == 1 and bwd(args(96), d=96) == 1
    odd = _Strides(H * S * D, S * D, D + 4)
    assert fwd(args(sq=odd)) == 1 and bwd(args(sq=odd)) == 1                # the plain entry points' checks
    assert fwd(args(H=3)) == 1 and bwd(args(H=3)) == 1
    assert bwd(args(), w=None) == 2                                         # GQA needs the workspace
    torch.cuda.synchronize(cuda)
    assert all(bool((t == GUARD16).all()) for t in outs) and all(bool((t == GUARD32).all()) for t in f32s)


# ------------------------------------------------------------------------- 5. the model, one captured step, executor
def _count(monkeypatch, lib):
    calls = {"plx_attn_fwd": 0, "plx_attn_bwd": 0, "plx_attn_drop_fwd": 0, "plx_attn_drop_bwd": 0}

    def wrap(name):
        real = getattr(lib, name)

        def f(*a):
            calls[name] += 1
            return real(*a)
        monkeypatch.setattr(lib, name, f)

    for name in calls:
        wrap(name)
    return calls


@pytest.mark.gpu
def test_feature_off_calls_the_plain_entry_points(cuda, monkeypatch):
    """The eager gpt2_tiny step (2 layers, one head of 64): without the state, and in eval(), only plx_attn_fwd /
    plx_attn_bwd are called; with it, only the DROP entry points."""
    from polyaxon_amd.ops import attention
    from polyaxon_amd.polyflow.programs import build_program

    calls = _count(monkeypatch, attention._lib())
    monkeypatch.setattr(attention, "_reference", lambda *a, **k: pytest.fail("the torch fallback ran"))

    def step(prog):
        prog.executor.reset(seed=0)
        prog.executor.set_hparams(**prog.info["warm_hparams"])
        prog.executor.run(1)
        torch.cuda.synchronize()

    plain = build_program("gpt2_tiny", {"graph": False, "heads": 1}, cuda)
    step(plain)
    assert calls == {"plx_attn_fwd": 2, "plx_attn_bwd": 2, "plx_attn_drop_fwd": 0, "plx_attn_drop_bwd": 0}
    prog = build_program("gpt2_tiny", {"graph": False, "heads": 1, "attn_dropout": True}, cuda)
    step(prog)
    assert calls == {"plx_attn_fwd": 2, "plx_attn_bwd": 2, "plx_attn_drop_fwd": 2, "plx_attn_drop_bwd": 2}
    model = prog.executor.model
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(prog.executor.x)
    model.train()
    torch.cuda.synchronize()
    assert calls == {"plx_attn_fwd": 4, "plx_attn_bwd": 2, "plx_attn_drop_fwd": 2, "plx_attn_drop_bwd": 2}
    model.set_attn_dropout(None)
    step(prog)
    assert calls == {"plx_attn_fwd": 6, "plx_attn_bwd": 4, "plx_attn_drop_fwd": 2, "plx_attn_drop_bwd": 2}


def _programs(cuda, extra, plain=None):
    """(plain program, program with ``extra``), both warmed, both captured or -- where the plain capture is rejected --
    both eager.  heads: 1 gives gpt2_tiny head_dim 64, so its attention runs the HIP kernels."""
    from polyaxon_amd.polyflow.programs import build_program

    params = {"graph": True, "heads": 1}
    if plain is not None:
        params["graph"] = plain.executor.graph is not None
    else:
        plain = build_program("gpt2_tiny", dict(params), cuda)
        plain.warm()
    if plain.executor.graph is None and params["graph"]:
        print("the plain gpt2_tiny capture was rejected here: both programs run eager")
        params = {"graph": False, "heads": 1}
        plain = build_program("gpt2_tiny", dict(params), cuda)
        plain.warm()
    prog = build_program("gpt2_tiny", dict(params, **extra), cuda)
    prog.warm()
    assert (prog.executor.graph is None) == (plain.executor.graph is None)
    return plain, prog


@pytest.mark.gpu
def test_one_captured_step_draws_fresh_masks_and_follows_the_rate(cuda, monkeypatch):
    """With the learning rate at 0 and the token stream rewound before every step, the weights and the batch are the
    same at every replay: the recorded loss then depends on the step counter and on the rate alone."""
    from polyaxon_amd.ops import attention

    monkeypatch.setattr(attention, "_reference", lambda *a, **k: pytest.fail("the torch fallback ran"))
    plain, prog = _programs(cuda, {"attn_dropout": True})
    ex0, ex = plain.executor, prog.executor
    graph = ex.graph
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k != "attn_dropout"}
    base.update(lr=0.0, weight_decay=0.0)
    c0 = ex.data.counter.clone()

    def losses(e, steps, first=0, **hp):
        e.reset(seed=3)
        e.set_hparams(**base, **hp)
        e.step.fill_(first)
        p0 = e.flat.params.clone()
        out = []
        for _ in range(steps):
            e.data.counter.copy_(c0)
            e.run(1)
            torch.cuda.synchronize()
            out.append(float(e.ring[(int(e.step.item()) - 1) % e.ring_size]))
        assert torch.equal(e.flat.params, p0)
        return out

    ref = losses(ex0, 3)
    assert ref[0] == ref[1] == ref[2]                        # no dropout: the same loss at every step
    assert losses(ex, 3, attn_dropout=0.0) == ref            # rate 0: bitwise the capture without the state
    half = losses(ex, 3, attn_dropout=0.5)
    assert len(set(half)) == 3 and ref[0] not in half        # a fresh mask at every replay
    assert losses(ex, 2, first=1, attn_dropout=0.5) == half[1:]   # ... drawn from the step counter
    quarter = losses(ex, 3, attn_dropout=0.25)               # one set, the same graph
    assert len(set(quarter + half)) == 6
    assert losses(ex, 3, attn_dropout=0.5) == half
    assert ex.graph is graph and ex.attn_dropout.hp.tolist()[0] == 128


@pytest.mark.gpu
def test_executor_searches_attn_dropout_in_one_captured_step(cuda, monkeypatch):
    from polyaxon_amd.ops import attention

    calls = _count(monkeypatch, attention._lib())
    monkeypatch.setattr(attention, "_reference", lambda *a, **k: pytest.fail("the torch fallback ran"))
    plain, prog = _programs(cuda, {"attn_dropout": True})
    assert calls["plx_attn_drop_fwd"] > 0 and calls["plx_attn_drop_bwd"] > 0
    assert prog.hp_keys == plain.hp_keys + ("attn_dropout",)
    ex0, ex = plain.executor, prog.executor
    assert ex0.attn_dropout is None and ex.dropout is None
    graph = ex.graph
    base = {k: v for k, v in prog.info["warm_hparams"].items() if k != "attn_dropout"}

    def trial(e, c0, seed, steps, **hp):
        e.data.counter.copy_(c0)
        e.reset(seed=seed)
        e.set_hparams(**base, **hp)
        e.run(steps)
        torch.cuda.synchronize()
        return e.flat.params.clone(), float(e.losses()[0])

    c0 = ex0.data.counter.clone()
    p0, l0 = trial(ex0, c0, 3, 3, attn_dropout=0.3)   # no param: the key is dropped
    p, l = trial(ex, c0, 3, 3, attn_dropout=0.0)
    assert torch.equal(p, p0) and l == l0              # rate 0: bitwise the plain program
    q, _ = trial(ex, c0, 3, 3, attn_dropout=0.3)
    assert ex.graph is graph                           # the same captured step
    assert not torch.equal(q, p) and bool(torch.isfinite(q).all())
    q2, _ = trial(ex, c0, 3, 3, attn_dropout=0.3)
    assert torch.equal(q2, q)

    # both dropouts in one captured step, each following its own key
    _, both = _programs(cuda, {"attn_dropout": True, "dropout": True}, plain)
    assert both.hp_keys == plain.hp_keys + ("dropout", "attn_dropout")
    eb = both.executor
    graph = eb.graph
    base = {k: v for k, v in both.info["warm_hparams"].items() if k not in ("attn_dropout", "dropout")}
    z, lz = trial(eb, c0, 3, 3, attn_dropout=0.0, dropout=0.0)
    assert torch.equal(z, p0) and lz == l0
    a, _ = trial(eb, c0, 3, 3, attn_dropout=0.3, dropout=0.0)
    assert torch.equal(a, q)                           # attention dropout alone: the program above
    r, _ = trial(eb, c0, 3, 3, attn_dropout=0.0, dropout=0.2)
    b, _ = trial(eb, c0, 3, 3, attn_dropout=0.3, dropout=0.2)
    assert len({t.cpu().numpy().tobytes() for t in (z, a, r, b)}) == 4 and bool(torch.isfinite(b).all())
    assert eb.graph is graph
