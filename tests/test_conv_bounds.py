"""The convolution GEMMs (csrc/conv_gemm.hip) on exact integer data and against derived per-element bounds.

tests/test_gpu_conv.py judges these kernels by assert_close with hand-picked tolerances, which accept a weight gradient
whose K-slice slabs are each rounded to bf16, one (tap, channel) term dropped from every output of a K = 4608
convolution, and a stats partial written to the neighbouring block row (test_old_tolerances_on_record keeps the record).
Here every output is compared with a plain fp64 reference written below (a shifted NHWC slice and an fp64 matmul per
tap, exact for bf16 inputs), on two kinds of data:

exact   small integers (activations / gradients in {-1, 0, 1} with ~3/4 zeros, weights in {-2..2}, integer D, integer
        mean, power-of-two invstd).  Every fp32 partial sum is an exact integer in any summation order, the float
        atomics of wgrad_kernel included, so fp32 outputs (weight gradients, stats rows, BatchNorm partial rows) must
        equal the reference bit for bit and bf16 outputs must equal torch's round-to-nearest-even of the exact value
        (with D: bf16(bf16(p) + d * mask), the kernel's two steps, :694).  The generator asserts sum |terms| < 2^24
        for everything it claims exact.  No element is excluded.
gauss   randn rounded to bf16; the statistic is max |got - ref| / bound and the assertion is <= 1.0; where the bound
        is 0 the element must be exact.

The bound, from the dataflow.  S = sum |a_k b_k| of an output element, U = 2^-8 (one bf16 store), E = 2^-23 per
addition inside an MFMA accumulation chain (the guides do not state the bf16 MFMA's internal rounding; 2^-23 holds
for round-to-nearest and for truncation, in any order), EV = 2^-24 per VALU fp32 addition (IEEE round-to-nearest)
and gamma(x) = x / (1 - x):
  NT product       (gemm_nt_kernel :528-:589, 2 MFMA steps of 32 per BK stage, acc in fp32): fp32 value within
                   gamma(K E) S, K the whole reduction (taps x channels); stored as bf16 by tile_to_lds (:623):
                   U |ref| + (1 + U) gamma(K E) S.
  D path           (:693-:708) the stored bf16 product q is read back, D * mask is added in fp32 and the sum is rounded
                   again: b1 = the line above, then b1 + (U + 2^-23) (|p + d| + b1).
  stats rows       (:677-:692, :730-:748) from the bf16 C the kernel stored: a thread adds ITERS = 8 rows in sequence,
                   then RSTEP (16 on the 128x128 tile, 32 on 256x64) per-thread sums are added in sequence:
                   gamma((ITERS + RSTEP) EV) sum |c|, and the same of sum c^2 (fmaf: one rounding per term).
  BN partials      (:710-:724) the same chain on sum |dz|; fmaf(g, (x - mu) * is, .) adds two roundings per term:
                   gamma((ITERS + RSTEP + 2) EV) sum |dz xhat|.  dz is the stored bf16 C (after D) under the mask.
  weight gradient  a term passes through the rows of one slice that one wave group accumulates (v2, wgrad_kernel
                   :1181-:1219: every KS-th 32-row stage of a kchunk-row slice; v1, gemm_tn_kernel :913-:955: all
                   kchunk rows), the KS - 1 group hand-offs (:1236-:1247), then the slices: the slab reducer's fp32
                   additions (:973-:1005) or one float atomic per slice (:1269, charged E each), plus one addition
                   into the base with accumulate.  kchunk and the slice count come from plx_tn_plan_slices (kchunk =
                   ceil(M / slices) rounded up to 32 KS rows, 64 for v1: tn2_plan :1527, tn_plan :1426).  The bound is
                   gamma(rows E + adds EV) (S + |base|).  A gamma(M) bound would accept a lost 32-row step of a
                   100352-row gradient; this one rejects it with ratio ~4 (test_chain_bound_rejects_a_lost_step).
  stem             forward as the NT product with K = 147 real products; its weight-gradient plan (block targets
                   kStemWgradBpc / kStemV2Bpc) is not exposed by the diagnostic, so the chain is the whole M (<= 1536
                   rows in the cases here) plus one addition per possible slice.

Layout: the oracle; an fp32 emulation of each dataflow (BK-stage order, tap-inner order, the two-step D add, K slices
and a slab sum) with the CPU tests -- the emulation is inside the bound and bit-exact on exact data, injected defects
are outside, the old tolerances' verdicts on those defects are on record, and every listed case reaches the
instantiation it is listed for (plx_gemm_nt_plan, plx_tn_plan_slices); then the GPU cases.

Largest measured ratio per kernel family on an MI355X (CONV_RATIO lines of the GPU cases; the fp32 emulation's over
the CPU-sized cases in brackets; every exact comparison was bit-equal):

    family            output        MI355X   emulation
    dense2            c             0.990    (0.986)     gemm_nt, NBUF 2 (K > 64, < 768 blocks)
    dense1            c             0.994    (0.869)     gemm_nt, NBUF 1 (K = 64; 768 blocks at K = 128, both tiles)
    conv2             c             0.990    (0.977)     plx_conv_fwd / plx_conv_dgrad, NBUF 2
    conv1             c             0.924    -           the same at >= 768 blocks, both tiles (GPU-sized cases only)
    dpath             c             0.983    (0.951)     D, D under a mask, D == dx in place
    stats             sum           0.016    (0.005)
    stats             sumsq         0.185    (0.163)
    bnpart            sum_dz        0.011    (0.000)
    bnpart            sum_dz_xhat   0.131    (0.088)
    wgrad_v1          dw            0.250    (0.005)     0.038 without the M = 1 cases
    wgrad_v2_slabs    dw            0.200    (0.022)     0.039
    wgrad_v2_atomic   dw            0.125    (0.022)     0.037
    stem              c             0.970    (0.957)
    stem              dw            0.043    (0.044)

The bf16 outputs sit at the bf16 rounding itself.  Below 0.05, and left there: stats sum and sum_dz add bf16 values, 8
significant bits each, so the fp32 partial sums of a block's <= 256 rows are exact unless the terms' exponents spread
over 16 bits -- on one-sign data (kind 'pos', sum c = sum |c|) the measured error is 0; the chain (ITERS + RSTEP) is
the kernel's own and sumsq, whose terms have 16 bits, uses a fifth of the same bound.  The weight gradients reach
0.12-0.25 only through the single addition into the base at M = 1; above one step they, like the stem's dw, use 0.04
of the bound on one-sign data and 0.025 on random signs.  Their chain is already the shortest the code supports (the
rows of one wave group of one slice, not M); what is left is the charge of one E per product inside an MFMA step, and
shortening that needs a statement on the bf16 MFMA's internal summation that neither guide makes and that must not be
read off the kernel under test.  What the bound does reject at that width is on record below: a lost 32-row step of
100352 rows (ratio ~4), a dropped slab, slabs rounded to bf16.
"""
import ctypes
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from polyaxon_amd.ops import _native

U = 2.0 ** -8             # bf16 round-to-nearest unit roundoff
E = 2.0 ** -23            # per addition of an MFMA accumulation chain, and per float atomic
EV = 2.0 ** -24           # per VALU fp32 addition
BF = torch.bfloat16
F64 = torch.float64
CUS = 256                 # MI355X; the CPU tests query the planner for it


def _gamma(x):
    return x / (1 - x)


def _lib():
    return _native.lib("plx_conv")


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode())


def _out(h, k, s):
    return (h + 2 * (k // 2) - k) // s + 1


def _rpb(n):
    """plx_gemm_nt_rows_per_block: rows of one stats / partial row."""
    return 128 if n % 128 == 0 else 256


def _row_chain(n):
    """ITERS + RSTEP of the NT epilogue (:600): RSTEP = 256 / (BN / 8)."""
    return 8 + (16 if n % 128 == 0 else 32)


# --------------------------------------------------------------------------------------------------------- the data
def _acts(kind, shape, g):
    """Activations / gradients, bf16."""
    if kind == "gauss":
        return torch.randn(shape, generator=g).to(BF)
    if kind == "pos":                                            # one sign: every partial sum is as large as S
        return torch.randn(shape, generator=g).abs().to(BF)
    r = torch.randint(0, 8, shape, generator=g)
    return torch.where(r == 0, 1.0, torch.where(r == 1, -1.0, 0.0)).to(BF)


def _weights(kind, shape, g):
    if kind == "gauss":
        return torch.randn(shape, generator=g).to(BF)
    if kind == "pos":
        return torch.randn(shape, generator=g).abs().to(BF)
    return torch.randint(-2, 3, shape, generator=g).float().to(BF)


def _addend(kind, shape, g):
    if kind != "exact":
        return (3.0 * torch.randn(shape, generator=g)).to(BF)
    return torch.randint(-4, 5, shape, generator=g).float().to(BF)


def _bn_inputs(kind, m, n, g):
    """x (bf16 [m][n]), mean, invstd (fp32 [n]) of the BatchNorm whose backward partials the epilogue reduces."""
    if kind != "exact":
        return (torch.randn(m, n, generator=g).to(BF), 0.3 * torch.randn(n, generator=g),
                0.5 + torch.rand(n, generator=g))
    return (torch.randint(-3, 4, (m, n), generator=g).float().to(BF), torch.randint(-1, 2, (n,), generator=g).float(),
            2.0 ** torch.randint(-1, 2, (n,), generator=g).float())


def _keep(shape, g):
    return torch.rand(shape, generator=g) > 0.5


def _pack_bits(keep):
    """[M][N] bool -> the 1-bit mask, bit k of byte i = element 8 i + k."""
    w = 2 ** torch.arange(8, dtype=torch.int32, device=keep.device)
    return (keep.reshape(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def _assert_exact_range(*sums):
    """Generator check: every fp32 partial sum of an 'exact' case is an integer below 2^24 (or a multiple of 1/4)."""
    for s in sums:
        assert float(s.max()) < 2 ** 24, float(s.max())


# ------------------------------------------------------------------------------------------------------- the oracle
# fp64, on whatever device the inputs live.  Activations are NHWC [Nb][H][W][C], weights [Cout][K*K][Cin] (the layout of
# Wf and of dW).  For each tap a shifted slice of the zero-padded tensor and one matmul; bf16 products are exact in fp64
# and the sums of <= 2^17 of them lose nothing that matters beside 2^-23.
def ref_nt(a, b):
    a, b = a.to(F64), b.to(F64)
    return a @ b.t(), a.abs() @ b.abs().t()


def _ref_fwd(x, w, k, s):
    nb, h, wd, _ = x.shape
    p, ho, wo = k // 2, _out(h, k, s), _out(wd, k, s)
    xp = F.pad(x, (0, 0, p, p, p, p))
    y = torch.zeros(nb, ho, wo, w.shape[0], dtype=F64, device=x.device)
    for kh in range(k):
        for kw in range(k):
            sl = xp[:, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s, :]
            y += sl @ w[:, kh * k + kw, :].t()
    return y


def ref_conv_fwd(x, w, k, s):
    """(y, S) [Nb][Ho][Wo][Cout]."""
    x, w = x.to(F64), w.to(F64)
    return _ref_fwd(x, w, k, s), _ref_fwd(x.abs(), w.abs(), k, s)


def _ref_dgrad(dy, w, k, s, h, wd):
    nb, ho, wo, _ = dy.shape
    p = k // 2
    dxp = torch.zeros(nb, h + 2 * p, wd + 2 * p, w.shape[2], dtype=F64, device=dy.device)
    for kh in range(k):
        for kw in range(k):
            dxp[:, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s, :] += dy @ w[:, kh * k + kw, :]
    return dxp[:, p:p + h, p:p + wd, :].contiguous()


def ref_conv_dgrad(dy, w, k, s, h, wd):
    """(dx, S) [Nb][H][W][Cin]: every output pixel's gradient scattered back through each tap."""
    dy, w = dy.to(F64), w.to(F64)
    return _ref_dgrad(dy, w, k, s, h, wd), _ref_dgrad(dy.abs(), w.abs(), k, s, h, wd)


def _ref_wgrad(dy, x, k, s):
    nb, ho, wo, co = dy.shape
    p = k // 2
    xp = F.pad(x, (0, 0, p, p, p, p))
    dw = torch.zeros(co, k * k, x.shape[3], dtype=F64, device=x.device)
    d2 = dy.reshape(-1, co)
    for kh in range(k):
        for kw in range(k):
            sl = xp[:, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s, :]
            dw[:, kh * k + kw, :] = d2.t() @ sl.reshape(-1, x.shape[3])
    return dw


def ref_conv_wgrad(dy, x, k, s):
    """(dW, S) [Cout][K*K][Cin]."""
    dy, x = dy.to(F64), x.to(F64)
    return _ref_wgrad(dy, x, k, s), _ref_wgrad(dy.abs(), x.abs(), k, s)


def ref_block_rows(v, rpb):
    """Per-block column sums of v [M][N] (fp64) in blocks of rpb rows: [nblk][N]."""
    m, n = v.shape
    nblk = -(-m // rpb)
    pad = torch.zeros(nblk * rpb, n, dtype=F64, device=v.device)
    pad[:m] = v
    return pad.view(nblk, rpb, n).sum(1)


def ref_stats(c, rpb):
    """Stats rows of the stored bf16 C: (sum c, sum c^2, sum |c|), each [nblk][N]."""
    c = c.to(F64)
    return ref_block_rows(c, rpb), ref_block_rows(c * c, rpb), ref_block_rows(c.abs(), rpb)


def ref_bn_terms(c, keep, x, mean, invstd):
    """dz and dz * xhat per element (fp64) from the stored C, the ReLU mask, and the BatchNorm's x / mean / invstd."""
    dz = c.to(F64) * keep.to(F64)
    return dz, dz * ((x.to(F64) - mean.to(F64)) * invstd.to(F64))


def dgrad_block_pixels(nb, h, w, k, s, rpb):
    """The pixels (flat NHW indices) behind each BatchNorm-partial block row of plx_conv_dgrad (:1903): one launch at
    stride 1; at stride 2 one per non-empty (ph, pw) parity class that has taps, in that order, each a row grid of its
    own pixels, and a partial row per rpb GEMM rows over all launches."""
    pix = torch.arange(nb * h * w).view(nb, h, w)
    launches = []
    if s == 1:
        launches.append(pix.reshape(-1))
    else:
        for ph in range(2):
            for pw in range(2):
                if k == 1 and (ph or pw):
                    continue                                  # a strided 1x1 reaches the even-even pixels only
                cls = pix[:, ph::2, pw::2].reshape(-1)
                if cls.numel():
                    launches.append(cls)
    return [l[i:i + rpb] for l in launches for i in range(0, l.numel(), rpb)]


# ------------------------------------------------------------------------------------------------------- the bounds
def bound_bf16(ref, s_abs, k):
    """One bf16 store of an fp32 MFMA sum of k products."""
    g = _gamma(k * E)
    return U * ref.abs() + (1 + U) * g * s_abs


def bound_dpath(p, s_abs, k, dm):
    b1 = bound_bf16(p, s_abs, k)
    return b1 + (U + 2.0 ** -23) * ((p + dm).abs() + b1)


def two_step(p, dm):
    """The D path on exact data: bf16(bf16(p) + d * mask), fp64 in and out."""
    q = p.float().to(BF).float()
    return (q + dm.float()).to(BF).to(F64)


def rne(p):
    return p.float().to(BF).to(F64)


def ratio(got, ref, bound):
    err = (got.to(ref.device).to(F64) - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


RATIOS = {}               # (family, output) -> the largest ratio check() has seen in this process


def check(kind, family, case, name, got, ref, bound, exact=None):
    """exact: bit equality with ``exact`` (default: the reference itself); else: ratio <= 1, printed first."""
    if kind == "exact":
        want = ref if exact is None else exact
        got64 = got.to(want.device).to(F64)
        bad = int((got64 != want).sum())
        assert bad == 0, f"{family} {case} {name}: {bad} of {want.numel()} elements differ on exact data, max " \
                         f"{float((got64 - want).abs().max())}"
        return 0.0
    r = ratio(got, ref, bound)
    print(f"CONV_RATIO {family} {case}-{kind} {name} {r:.4f}")
    RATIOS[family, name] = max(RATIOS.get((family, name), 0.0), r)
    assert r <= 1.0, f"{family} {case} {name}: ratio {r}"
    return r


# ---------------------------------------------------------------------------------- the weight-gradient plan's model
def v2_cfg(n1, n2):
    """(NA, NB, KS) of wgrad_kernel for an N1 x N2 output (v2_cfg :1459; the table of the GPU cases pins it)."""
    if n1 % 128 == 0 and n2 % 128 == 0:
        return 2, 2, 2
    if n1 % 128 != 0:
        if n1 == 64 and n2 % 256 == 0:
            return 1, 4, 2
        if n1 == 64 and n2 % 192 == 0:
            return 1, 3, 2
        if n1 == 64 and n2 % 128 == 0:
            return 1, 2, 4
        return 1, 1, 8
    return (4, 1, 2) if n1 % 256 == 0 else (2, 1, 4)


# hook settings (plx_set_tn_v2 on, ring KB; plx_set_tn_atomic; plx_set_tn2_c64) -> family
HOOKS = {"v1": (0, -1, 1, 1), "v2_64k_atomic": (1, 64, 1, 1), "v2_128k_atomic": (1, 128, 1, 1),
         "v2_64k_slabs": (1, 64, 0, 1), "v2_128k_slabs": (1, 128, 0, 1), "v2_no6wave": (1, 64, 1, 0)}


def tn_model(m, n1, n2, hook, cus=CUS):
    """(family, ks, kchunk, slices, mfma rows, valu adds, atomic adds) of the weight gradient the hooks select."""
    on, _, atomic, c64 = HOOKS[hook]
    na, nb, ks = v2_cfg(n1, n2)
    v2 = on == 1 and not (na == 1 and nb == 3 and not c64)
    slices = _lib().plx_tn_plan_slices(m, n1, n2, cus, 1 if v2 else 0)
    assert slices >= 1
    step = 32 * ks if v2 else 64
    kchunk = -(-(-(-m // slices)) // step) * step
    assert -(-m // kchunk) == slices, (m, slices, kchunk)
    if not v2:
        return "wgrad_v1", 1, kchunk, slices, min(kchunk, m), slices, 0
    rows = min(32 * -(-(kchunk // 32) // ks), m)
    if atomic:
        return "wgrad_v2_atomic", ks, kchunk, slices, rows, ks - 1, slices + 1
    return "wgrad_v2_slabs", ks, kchunk, slices, rows, ks - 1 + slices, 0


def bound_wgrad(s_abs, base_abs, model, accumulate):
    _, _, _, _, rows, adds, atom = model
    return _gamma(rows * E + atom * E + (adds + (1 if accumulate else 0)) * EV) * (s_abs + base_abs)


def bound_stem_dw(s_abs, m):
    """The stem's weight gradient: its plans (tn_plan with kStemWgradBpc, tn2_plan with kStemV2Bpc) are not behind the
    diagnostic, so every row of M is charged to one chain, one E per slice a plan could make (>= 256 rows each: by_depth
    :1421, :1515), the wave-group hand-off and the unpack's addition."""
    return _gamma((m + m // 256 + 1) * E + 2 * EV) * s_abs


def ragged_m(n1, n2, hook="v2_64k_atomic", cus=CUS):
    """The smallest M whose plan has >= 2 slices and a ragged last one."""
    ks = v2_cfg(n1, n2)[2]
    m = 4 * 32 * ks
    while True:
        m += 1
        mod = tn_model(m, n1, n2, hook, cus)
        if mod[3] >= 2 and m % mod[2] != 0:
            return m


def wgrad_ms(n1, n2):
    ks = v2_cfg(n1, n2)[2]
    return [1, 31, 32, 33, 32 * ks * 4 - 1, 32 * ks * 4 + 1, ragged_m(n1, n2)]


WGRAD_PAIRS = {(128, 128): (2, 2, 2), (64, 256): (1, 4, 2), (64, 192): (1, 3, 2), (64, 128): (1, 2, 4),
               (64, 64): (1, 1, 8), (192, 64): (1, 1, 8), (256, 64): (4, 1, 2), (128, 64): (2, 1, 4)}
# (Cin, Cout, K, S): N1 = Cout, N2 = K K Cin
WGRAD_CONVS = [(64, 64, 3, 1), (64, 128, 3, 1), (64, 256, 3, 1), (128, 64, 3, 1), (128, 128, 3, 1), (64, 64, 3, 2),
               (128, 128, 3, 2), (64, 128, 1, 2), (128, 64, 1, 2), (64, 64, 1, 2)]
WGRAD_CONV_SHAPES = [(2, 13, 9), (3, 31, 23)]


# ------------------------------------------------------------------------------- the fp32 emulation of the dataflows
def gather_idx(nb, hs, ws, hr, wr, s, offs, defect=None):
    """The kernel's row -> source pixel map (:267-:282): [taps][M] flat source rows of an hs x ws image for the rows of
    an hr x wr grid, -1 outside the image.  Defects: 'wrap' lets a tap one past the right edge read the next row's
    first pixel; 'top' lets a tap above the top border read the row before it in memory."""
    m = torch.arange(nb * hr * wr)
    c, q = m % wr, m // wr
    r, n = q % hr, q // hr
    out = []
    for dh, dw in offs:
        ih, iw = r * s + dh, c * s + dw
        okh, okw = (ih >= 0) & (ih < hs), (iw >= 0) & (iw < ws)
        if defect == "wrap":
            okw = iw >= 0
        if defect == "top":
            okh = ih < hs
        src = (n * hs + ih) * ws + iw
        ok = okh & okw & (src >= 0) & (src < nb * hs * ws)
        out.append(torch.where(ok, src, torch.full_like(src, -1)))
    return torch.stack(out)


def im2col(rows, idx, tap_inner):
    """[M][taps * C] gathered operand; tap_inner: columns in the NT kernels' stage order (all taps of a 64-channel
    chunk back to back, :353), else tap-major (the weight gradient's N2 index)."""
    t, m = idx.shape
    c = rows.shape[1]
    a = rows[idx.clamp_min(0)] * (idx >= 0).unsqueeze(-1).to(rows.dtype)            # [T][M][C]
    if tap_inner and c % 64 == 0:
        return a.view(t, m, c // 64, 64).permute(1, 2, 0, 3).reshape(m, t * c)
    return a.permute(1, 0, 2).reshape(m, t * c)


def wcols(w, tap_inner):
    """[N][taps][C] -> [N][taps * C] in the same column order."""
    n, t, c = w.shape
    if tap_inner and c % 64 == 0:
        return w.view(n, t, c // 64, 64).permute(0, 2, 1, 3).reshape(n, t * c)
    return w.reshape(n, t * c)


def emu_acc(am, bm):
    """fp32 accumulation over 32-deep MFMA steps in column order."""
    kp = am.shape[1]
    if kp % 32:
        am, bm = F.pad(am, (0, 32 - kp % 32)), F.pad(bm, (0, 32 - kp % 32))
    acc = torch.zeros(am.shape[0], bm.shape[0], dtype=torch.float32)
    for k0 in range(0, am.shape[1], 32):
        acc = acc + am[:, k0:k0 + 32].float() @ bm[:, k0:k0 + 32].float().t()
    return acc


def emu_store(acc, d=None, keep=None):
    """tile_to_lds rounds to bf16; the D path adds D * mask to that in fp32 and rounds again.  Returns (q, out)."""
    q = acc.to(BF)
    if d is None:
        return q, q
    dm = d.float() if keep is None else d.float() * keep.float()
    return q, (q.float() + dm).to(BF)


def fwd_offs(k):
    return [(t // k - k // 2, t % k - k // 2) for t in range(k * k)]


def emu_conv_fwd(x, w, k, s, defect=None):
    """fp32 acc [M][Cout] of the forward in the NT kernel's order."""
    nb, h, wd, c = x.shape
    idx = gather_idx(nb, h, wd, _out(h, k, s), _out(wd, k, s), s, fwd_offs(k), defect)
    return emu_acc(im2col(x.reshape(-1, c), idx, True), wcols(w, True))


def emu_conv_dgrad(dy, w, k, s, h, wd, defect=None):
    """fp32 acc [Nb*H*W][Cin] of the data gradient: stride 1 gathers dy through the flipped taps; stride 2 runs one
    GEMM per parity class over the taps of matching parity and scatters its rows (:1863).  Pixels no class reaches
    stay NaN.  Defect 'parity': class (0, 1) lands on the pixels of class (1, 0)."""
    nb, ho, wo, co = dy.shape
    p, cin = k // 2, w.shape[2]
    wdt = w.permute(2, 1, 0).contiguous()                       # Wd [Cin][taps][Cout]
    rows = dy.reshape(-1, co)
    if s == 1:
        idx = gather_idx(nb, ho, wo, h, wd, 1, [(p - t // k, p - t % k) for t in range(k * k)], defect)
        return emu_acc(im2col(rows, idx, True), wcols(wdt, True))
    out = torch.full((nb, h, wd, cin), math.nan, dtype=torch.float32)
    for ph in range(2):
        for pw in range(2):
            taps = [(kh, kw) for kh in range(k) for kw in range(k)
                    if (ph + p - kh) % 2 == 0 and (pw + p - kw) % 2 == 0]
            hr, wr = (h - ph + 1) // 2, (wd - pw + 1) // 2
            if not taps or hr <= 0 or wr <= 0:
                continue
            idx = gather_idx(nb, ho, wo, hr, wr, 1, [((ph + p - kh) // 2, (pw + p - kw) // 2) for kh, kw in taps])
            wsel = wdt[:, [kh * k + kw for kh, kw in taps], :].contiguous()
            acc = emu_acc(im2col(rows, idx, True), wcols(wsel, True)).view(nb, hr, wr, cin)
            if defect == "parity" and (ph, pw) == (0, 1):
                out[:, 1::2, 0::2, :] = acc
            else:
                out[:, ph::2, pw::2, :] = acc
    return out.view(-1, cin)


def emu_tn(a, b, kchunk, ks, stage=32, drop_slab=None, bf16_slabs=False, base=None):
    """fp32 [N1][N2] of the weight gradient: per K slice, wave group g adds every ks-th ``stage``-row step in sequence,
    the groups are added in order, and the slices are added in order (slabs or atomics) onto the base."""
    m = a.shape[0]
    out = torch.zeros(a.shape[1], b.shape[1]) if base is None else base.clone().float()
    for si, k0 in enumerate(range(0, m, kchunk)):
        k1 = min(m, k0 + kchunk)
        groups = []
        for g in range(ks):
            acc = torch.zeros(a.shape[1], b.shape[1])
            for r0 in range(k0 + g * stage, k1, ks * stage):
                for q0 in range(r0, min(r0 + stage, k1), 32):
                    acc = acc + a[q0:min(q0 + 32, k1)].float().t() @ b[q0:min(q0 + 32, k1)].float()
            groups.append(acc)
        slab = groups[0]
        for gacc in groups[1:]:
            slab = slab + gacc
        if bf16_slabs:
            slab = slab.to(BF).float()
        if si != drop_slab:
            out = out + slab
    return out


def emu_block_sums(v, rpb, n_cols, second=None):
    """The epilogue's per-block column sums in thread order (:677, :743): thread j of a chunk column adds rows
    j, j + RSTEP, ... in sequence, then the RSTEP thread sums are added in sequence.  v [M][N] fp32 terms; with
    ``second`` the term is fmaf(v, second, .): one rounding per addition."""
    rstep = 16 if n_cols % 128 == 0 else 32
    m, n = v.shape
    nblk = -(-m // rpb)

    def padded(t):
        z = torch.zeros(nblk * rpb, n, dtype=torch.float32)
        z[:m] = t
        return z.view(nblk, rpb // rstep, rstep, n)
    pv, ps = padded(v), (padded(second) if second is not None else None)
    th = torch.zeros(nblk, rstep, n)
    for it in range(rpb // rstep):
        if ps is None:
            th = th + pv[:, it]
        else:
            th = (th.double() + pv[:, it].double() * ps[:, it].double()).float()
    tot = torch.zeros(nblk, n)
    for j in range(rstep):
        tot = tot + th[:, j]
    return tot


def emu_stats(q, n_cols):
    qf = q.float()
    return emu_block_sums(qf, _rpb(n_cols), n_cols), emu_block_sums(qf, _rpb(n_cols), n_cols, qf)


def skip_mask(m, sh, sw, odd=False):
    """Rows of even-even pixels of [n][sh][sw] images (BnBwd::skip_w, :660); odd: the defect, odd-odd pixels."""
    gm = torch.arange(m)
    col, row = gm % sw, (gm // sw) % sh
    return ((col % 2 == 1) & (row % 2 == 1)) if odd else ((col % 2 == 0) & (row % 2 == 0))


def emu_bn_partials(out, keep, x, mean, invstd, n_cols, skip=None):
    g = out.float() * keep.float()
    if skip is not None:
        g = g * (~skip).float().unsqueeze(1)
    xh = (x.float() - mean) * invstd
    return emu_block_sums(g, _rpb(n_cols), n_cols), emu_block_sums(g, _rpb(n_cols), n_cols, xh)


# ------------------------------------------------------------------------------------ one checked GEMM, CPU or GPU
def judge_nt(kind, family, case, p, s_abs, k, q_got, out_got, d=None, keep=None, stats_got=None, bn=None, part_got=None,
             skip=None, block_rows=None, judge_c=True):
    """Hold the outputs of one NT GEMM (dense or gathered) to the oracle.  p, s_abs: fp64 [M][N]; q_got: the stored
    product when no D is added (else None); out_got: the stored C; stats_got [2][nblk][N]; bn = (x, mean, invstd) and
    part_got [2][nblk][N]; block_rows: the rows behind each partial row (default: consecutive rpb-row blocks)."""
    dev = p.device
    n = p.shape[1]
    if d is not None:
        dm = d.to(dev).to(F64) * (keep.to(dev).to(F64) if keep is not None else 1.0)
        if judge_c:
            check(kind, "dpath", case, "c", out_got, p + dm, bound_dpath(p, s_abs, k, dm),
                  two_step(p, dm))
    elif judge_c:
        check(kind, family, case, "c", out_got, p, bound_bf16(p, s_abs, k), rne(p))
    stored = out_got.to(dev)
    chain = _row_chain(n)
    if stats_got is not None:
        s1, s2, sabs = ref_stats(stored if q_got is None else q_got.to(dev), _rpb(n))
        if kind == "exact":
            _assert_exact_range(sabs, s2)
        g = _gamma(chain * EV)
        check(kind, "stats", case, "sum", stats_got[0], s1, g * sabs)
        check(kind, "stats", case, "sumsq", stats_got[1], s2, g * s2)
    if bn is not None:
        x, mean, invstd = (t.to(dev) for t in bn)
        kp = keep.to(dev) if keep is not None else torch.ones_like(p, dtype=torch.bool)
        if skip is not None:
            kp = kp & ~skip.to(dev).unsqueeze(1)
        dz, dzx = ref_bn_terms(stored, kp, x, mean, invstd)
        if block_rows is None:
            ra, rb = ref_block_rows(dz, _rpb(n)), ref_block_rows(dzx, _rpb(n))
            aa, ab = ref_block_rows(dz.abs(), _rpb(n)), ref_block_rows(dzx.abs(), _rpb(n))
        else:
            rows = [r.to(dev) for r in block_rows]
            ra, rb = torch.stack([dz[r].sum(0) for r in rows]), torch.stack([dzx[r].sum(0) for r in rows])
            aa = torch.stack([dz[r].abs().sum(0) for r in rows])
            ab = torch.stack([dzx[r].abs().sum(0) for r in rows])
        if kind == "exact":
            _assert_exact_range(aa, 4 * ab)
        check(kind, "bnpart", case, "sum_dz", part_got[0], ra, _gamma(chain * EV) * aa)
        check(kind, "bnpart", case, "sum_dz_xhat", part_got[1], rb, _gamma((chain + 2) * EV) * ab)


# ----------------------------------------------------------------------------------------------------- the CPU cases
CPU_DENSE = [(1, 64, 64), (129, 128, 192), (300, 192, 128), (257, 256, 576)]
# (K, S, Nb, Cin, Cout, H, W)
CPU_CONV = [(3, 1, 3, 128, 128, 9, 11), (3, 1, 1, 64, 192, 1, 5), (3, 2, 3, 64, 128, 7, 9), (3, 2, 1, 128, 64, 5, 1),
            (1, 2, 3, 64, 64, 8, 8), (3, 2, 2, 64, 64, 8, 8), (3, 1, 1, 64, 64, 2, 300)]
CPU_WGRAD = [(333, 64, 64), (1025, 128, 128), (2049, 64, 192), (1100, 256, 64)]
CPU_STEM = [(1, 2, 2), (1, 8, 6), (2, 33, 18)]
KINDS = ("exact", "gauss")
KINDS_W = ("exact", "gauss", "pos")                               # the weight gradients also on one-sign data


def _dense_inputs(kind, m, n, k, g):
    return _acts(kind, (m, k), g), _weights(kind, (n, k), g)


def _emu_dense_case(kind, m, n, k):
    g = torch.Generator().manual_seed(_seed("dense", m, n, k, kind))
    a, b = _dense_inputs(kind, m, n, k, g)
    d, keep = _addend(kind, (m, n), g), _keep((m, n), g)
    bn = _bn_inputs(kind, m, n, g)
    p, s_abs = ref_nt(a, b)
    if kind == "exact":
        _assert_exact_range(s_abs)
    acc = emu_acc(a, b)
    case = f"emu-dense-{m}x{n}x{k}"
    fam = "dense1" if k == 64 else "dense2"
    q, _ = emu_store(acc)
    judge_nt(kind, fam, case, p, s_abs, k, q, q, stats_got=torch.stack(emu_stats(q, n)))
    q, out = emu_store(acc, d, keep)
    skip = skip_mask(m, 3, 5)
    part = torch.stack(emu_bn_partials(out, keep, *bn, n, skip))
    judge_nt(kind, fam, case, p, s_abs, k, None, out, d, keep, bn=bn, part_got=part, skip=skip)


def _conv_inputs(kind, k, s, nb, cin, cout, h, w, g):
    x = _acts(kind, (nb, h, w, cin), g)
    wt = _weights(kind, (cout, k * k, cin), g)
    dy = _acts(kind, (nb, _out(h, k, s), _out(w, k, s), cout), g)
    return x, wt, dy


def _emu_conv_case(kind, cfg):
    k, s, nb, cin, cout, h, w = cfg
    g = torch.Generator().manual_seed(_seed("conv", cfg, kind))
    x, wt, dy = _conv_inputs(kind, k, s, nb, cin, cout, h, w, g)
    case = "emu-conv-" + "x".join(map(str, cfg))
    y, sy = ref_conv_fwd(x, wt, k, s)
    y, sy = y.view(-1, cout), sy.view(-1, cout)
    if kind == "exact":
        _assert_exact_range(sy)
    q, _ = emu_store(emu_conv_fwd(x, wt, k, s))
    judge_nt(kind, "conv2", case, y, sy, k * k * cin, q, q, stats_got=torch.stack(emu_stats(q, cout)))
    dx, sx = ref_conv_dgrad(dy, wt, k, s, h, w)
    dx, sx = dx.view(-1, cin), sx.view(-1, cin)
    acc = emu_conv_dgrad(dy, wt, k, s, h, w)
    if k == 1 and s == 2:                                       # only the even-even pixels are written
        written = skip_mask(nb * h * w, h, w)
        assert bool(torch.isnan(acc[~written]).all()) and not bool(torch.isnan(acc[written]).any())
        acc, dx, sx = acc[written], dx[written], sx[written]
    q, _ = emu_store(acc)
    judge_nt(kind, "conv2", case + "-dgrad", dx, sx, k * k * cout, q, q)


def _emu_wgrad_case(kind, m, n1, n2, hook):
    g = torch.Generator().manual_seed(_seed("wgrad", m, n1, n2, kind))
    a, b = _acts(kind, (m, n1), g), _acts(kind, (m, n2), g)
    base = _addend(kind, (n1, n2), g).float()
    mod = tn_model(m, n1, n2, hook)
    ref = a.to(F64).t() @ b.to(F64)
    s_abs = a.to(F64).abs().t() @ b.to(F64).abs()
    if kind == "exact":
        _assert_exact_range(s_abs + base.abs())
    got = emu_tn(a, b, mod[2], mod[1], 64 if mod[0] == "wgrad_v1" else 32, base=base)
    check(kind, mod[0], f"emu-tn-{m}x{n1}x{n2}-{hook}", "dw", got, ref + base.to(F64),
              bound_wgrad(s_abs, base.to(F64).abs(), mod, True))


def stem_weight_taps(w):
    """[64][3][7][7] -> [64][49][3]."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 49, 3)


def _emu_stem_case(kind, shape):
    nb, h, w = shape
    g = torch.Generator().manual_seed(_seed("stem", shape, kind))
    x, wt, dy = _conv_inputs(kind, 7, 2, nb, 3, 64, h, w, g)
    y, sy = ref_conv_fwd(x, wt, 7, 2)
    y, sy = y.view(-1, 64), sy.view(-1, 64)
    idx = gather_idx(nb, h, w, _out(h, 7, 2), _out(w, 7, 2), 2, fwd_offs(7))
    am = im2col(x.reshape(-1, 3), idx, False)
    q, _ = emu_store(emu_acc(am, wcols(wt, False)))
    case = f"emu-stem-{nb}x{h}x{w}"
    judge_nt(kind, "stem", case, y, sy, 147, q, q, stats_got=torch.stack(emu_stats(q, 64)))
    dw, sw = ref_conv_wgrad(dy, x, 7, 2)
    m = y.shape[0]
    got = emu_tn(dy.reshape(-1, 64), am, 64 * -(-m // 64), 1, 64)
    check(kind, "stem", case, "dw", got, dw.view(64, -1), bound_stem_dw(sw.view(64, -1), m))


def test_emulation_is_inside_the_bound_and_exact_on_integers():
    """The fp32 emulation of every dataflow: ratio <= 1 on the gauss cases, bit-equal on the exact ones."""
    RATIOS.clear()
    for kind in KINDS:
        for m, n, k in CPU_DENSE:
            _emu_dense_case(kind, m, n, k)
            if kind == "gauss":
                _emu_dense_case("pos", m, n, k)
        for cfg in CPU_CONV:
            _emu_conv_case(kind, cfg)
        for m, n1, n2 in CPU_WGRAD:
            for hook in ("v1", "v2_64k_atomic", "v2_64k_slabs"):
                _emu_wgrad_case(kind, m, n1, n2, hook)
                if kind == "gauss":
                    _emu_wgrad_case("pos", m, n1, n2, hook)
        for shape in CPU_STEM:
            _emu_stem_case(kind, shape)
    print("CONV_EMU_WORST", {f"{f}.{o}": round(r, 3) for (f, o), r in sorted(RATIOS.items())})
    assert RATIOS and max(RATIOS.values()) <= 1.0


# --------------------------------------------------------------------------------------------------- injected defects
def _fwd_defect(kind, defect):
    """(got, ref, bound, exact) of the (3,128,9,11) -> 128 3x3 forward computed with a defect."""
    cfg = (3, 1, 3, 128, 128, 9, 11)
    k, s, nb, cin, cout, h, w = cfg
    g = torch.Generator().manual_seed(_seed("defect", kind))
    x, wt, _ = _conv_inputs(kind, k, s, nb, cin, cout, h, w, g)
    y, sy = ref_conv_fwd(x, wt, k, s)
    y, sy = y.view(-1, cout), sy.view(-1, cout)
    if defect == "term":                                        # one (tap, channel) term of one output element
        idx = gather_idx(nb, h, w, h, w, 1, fwd_offs(k))
        am, bm = im2col(x.reshape(-1, cin), idx, True), wcols(wt, True)
        acc = emu_acc(am, bm)
        m0, n0 = 100, 7
        nz = torch.nonzero((am[m0].float() != 0) & (bm[n0].float() != 0)).flatten()
        acc[m0, n0] -= am[m0, nz[0]].float() * bm[n0, nz[0]].float()
    else:
        acc = emu_conv_fwd(x, wt, k, s, None if defect == "ragged" else defect)
        if defect == "ragged":
            acc[-1] = acc[-2]
    q, _ = emu_store(acc)
    return q, y, bound_bf16(y, sy, k * k * cin), rne(y)


def _outside(kind, got, ref, bound, exact):
    if kind == "exact":
        return bool((got.to(F64) != (ref if exact is None else exact)).any())
    return ratio(got, ref, bound) > 1.0


@pytest.mark.parametrize("defect", ["term", "wrap", "top", "ragged"])
def test_forward_defects_are_outside(defect):
    """A dropped (tap, channel) term of one element, a right-edge tap that wraps to the next row's first pixel, a
    top-border tap not zeroed, the last row taken from row M - 2: each fails the exact comparison, and each but the
    single dropped term (one product of 1152, below the bf16 rounding of its element) exceeds the gauss bound."""
    assert _outside("exact", *_fwd_defect("exact", defect))
    got, ref, bound, _ = _fwd_defect("gauss", defect)
    r = ratio(got, ref, bound)
    print(f"CONV_DEFECT {defect} gauss ratio {r:.3f}")
    if defect != "term":
        assert r > 1.0


def test_parity_class_scattered_to_the_wrong_pixels_is_outside():
    k, s, nb, cin, cout, h, w = 3, 2, 2, 64, 64, 8, 8
    for kind in KINDS:
        g = torch.Generator().manual_seed(_seed("parity", kind))
        _, wt, dy = _conv_inputs(kind, k, s, nb, cin, cout, h, w, g)
        dx, sx = ref_conv_dgrad(dy, wt, k, s, h, w)
        dx, sx = dx.view(-1, cin), sx.view(-1, cin)
        q, _ = emu_store(torch.nan_to_num(emu_conv_dgrad(dy, wt, k, s, h, w, "parity"), nan=0.0))
        assert _outside(kind, q, dx, bound_bf16(dx, sx, k * k * cout), rne(dx)), kind


@pytest.mark.parametrize("defect", ["drop_slab", "bf16_slabs"])
def test_slab_defects_are_outside(defect):
    m, n1, n2 = 2049, 64, 192
    for kind in KINDS:
        g = torch.Generator().manual_seed(_seed("slab", kind))
        a, b = _acts(kind, (m, n1), g), _acts(kind, (m, n2), g)
        if kind == "exact" and defect == "bf16_slabs":           # sums past 256 so that a bf16 slab loses integers
            a, b = a.abs() * 3, b.abs() * 3
        mod = tn_model(m, n1, n2, "v2_64k_slabs")
        assert mod[3] >= 2
        ref, s_abs = a.to(F64).t() @ b.to(F64), a.to(F64).abs().t() @ b.to(F64).abs()
        got = emu_tn(a, b, mod[2], mod[1], drop_slab=1 if defect == "drop_slab" else None,
                     bf16_slabs=defect == "bf16_slabs")
        assert _outside(kind, got, ref, bound_wgrad(s_abs, 0.0, mod, False), None), kind


def test_partials_on_the_wrong_rows_are_outside():
    """A stats partial written to the neighbouring block row, and the even-even skip applied to the odd pixels."""
    m, n, k = 700, 128, 128
    for kind in KINDS:
        g = torch.Generator().manual_seed(_seed("rows", kind))
        a, b = _dense_inputs(kind, m, n, k, g)
        keep, bn = _keep((m, n), g), _bn_inputs(kind, m, n, g)
        q, _ = emu_store(emu_acc(a, b))
        s1, s2, sabs = ref_stats(q, _rpb(n))
        st = emu_stats(q, n)[0]
        st[[1, 2]] = st[[2, 1]]
        assert _outside(kind, st, s1, _gamma(_row_chain(n) * EV) * sabs, None), kind
        skip = skip_mask(m, 10, 7)
        part = emu_bn_partials(q, keep, *bn, n, skip_mask(m, 10, 7, odd=True))[0]
        dz, _ = ref_bn_terms(q, keep & ~skip.unsqueeze(1), *bn)
        assert _outside(kind, part, ref_block_rows(dz, _rpb(n)),
                        _gamma(_row_chain(n) * EV) * ref_block_rows(dz.abs(), _rpb(n)), None), kind


def test_chain_bound_rejects_a_lost_step():
    """A whole 32-row step lost from one slice of a 100352-row weight gradient (the 56x56 layers): gamma(M) S accepts
    it, the chain-aware bound does not."""
    m, n1, n2 = 100352, 64, 64
    g = torch.Generator().manual_seed(5)
    a, b = _acts("gauss", (m, n1), g).to(F64), _acts("gauss", (m, n2), g).to(F64)
    ref, s_abs = a.t() @ b, a.abs().t() @ b.abs()
    lost = ref - a[5000:5032].t() @ b[5000:5032]
    mod = tn_model(m, n1, n2, "v2_64k_atomic")
    assert ratio(lost, ref, _gamma(m * E) * s_abs) <= 1.0
    assert ratio(lost, ref, bound_wgrad(s_abs, 0.0, mod, False)) > 2.0


def _old_ok(got, ref, rtol, atol):
    return bool(((got.to(F64) - ref).abs() <= atol + rtol * ref.abs()).all())


def test_old_tolerances_on_record():
    """What the assert_close settings of tests/test_gpu_conv.py make of the defects above.  Accepted: a weight gradient
    whose ~190 K-slice slabs are rounded to bf16 (rtol 2e-2, atol 2e-2 max |ref|: test_wgrad_kernels_every_class), one
    (tap, channel) term dropped from EVERY element of the (5,512,7,7) -> 512 3x3 forward (K = 4608; rtol 2e-2, atol
    8e-2: test_conv_implicit_gemm_matches_fp32), and a stats row written to the neighbouring block (only the sum over
    blocks and block 0 are compared: test_gemm_nt_channel_stats).  Rejected: the right-edge wrap and a dropped
    64-channel stage on the same forward shapes."""
    g = torch.Generator().manual_seed(5)
    m = 100352 // 4                                             # 48 slices' worth is enough to show it
    a, b = _acts("gauss", (m, 64), g).to(F64), _acts("gauss", (m, 64), g).to(F64)
    ref = a.t() @ b
    slabs = torch.stack([(a[i::48].t() @ b[i::48]).float().to(BF).to(F64) for i in range(48)]).sum(0)
    assert _old_ok(slabs, ref, 2e-2, 2e-2 * float(ref.abs().max()))
    x, wt, _ = _conv_inputs("gauss", 3, 1, 5, 512, 512, 7, 7, g)
    wt = ((2 * torch.rand(wt.shape, generator=g) - 1) / 4608 ** 0.5).to(BF)   # a Conv2d's default init
    y, _ = ref_conv_fwd(x, wt, 3, 1)
    one = x.to(F64)[..., 7:8] @ wt.to(F64)[:, 4, 7:8].t()        # centre tap, channel 7, every element
    assert _old_ok(rne(y - one), y, 2e-2, 8e-2)
    stage = x.to(F64)[..., :64] @ wt.to(F64)[:, 4, :64].t()      # one BK stage: centre tap, 64 channels
    assert not _old_ok(rne(y - stage), y, 2e-2, 8e-2)
    got, ref_w, _, _ = _fwd_defect("gauss", "wrap")
    assert not _old_ok(got, ref_w, 2e-2, 8e-2)
    a, b = _dense_inputs("gauss", 777, 128, 128, g)
    q = rne(ref_nt(a, b)[0])
    s1 = ref_block_rows(q, 128)
    moved = s1.clone()
    moved[[1, 2]] = s1[[2, 1]]                                  # the old test: the sum over blocks, and block 0
    assert torch.allclose(moved.sum(0), q.sum(0), rtol=1e-4, atol=1e-2) and torch.equal(moved[0], q[:128].sum(0))
    assert not torch.equal(moved, s1)


# ------------------------------------------------------------------------------------------------------- case tables
DENSE_MS = [1, 127, 128, 129, 255, 256, 257, 300]
DENSE_NS = [64, 128, 192, 256]
DENSE_KS = [64, 128, 192, 576]
DENSE_BIG = [(24571, 512, 128, 1128), (65531, 192, 128, 1256)]
CONV_MODES = [(3, 1), (3, 2), (1, 2)]
CONV_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (7, 9), (8, 8), (13, 9), (5, 17), (2, 300)]
CONV_COMBOS = [(cin, cout, nb) for cin in (64, 128) for cout in (64, 128, 192) for nb in (1, 3)]
# (K, S, Nb, Cin, Cout, H, W, forward plan or None, data-gradient plan or None)
CONV_BIG = [(3, 1, 1, 64, 512, 157, 157, 1128, None), (3, 1, 1, 512, 64, 157, 157, None, 1128),
            (3, 1, 1, 64, 192, 255, 257, 1256, None), (3, 1, 1, 192, 64, 255, 257, None, 1256)]
STEM_SHAPES = [(1, 2, 2), (1, 8, 6), (2, 33, 18), (2, 64, 48)]


def conv_cases(mode_i, size_i):
    """Two (Cin, Cout, Nb) combinations per (mode, size): over the ten sizes every combination meets every mode."""
    return [CONV_COMBOS[(size_i + 3 * mode_i) % 12], CONV_COMBOS[(size_i + 3 * mode_i + 6) % 12]]


def test_case_tables_reach_their_instantiations():
    """plx_gemm_nt_plan: the small dense and gathered cases run NBUF = 2 (dense K = 64: NBUF = 1), the large ones
    NBUF = 1 on the tile they are listed for; the (N1, N2) pairs reach every v2 configuration; ragged_m gives >= 2
    slices with a ragged last one."""
    lib = _lib()
    for n in DENSE_NS:
        bm = 128 if n % 128 == 0 else 256
        for k in DENSE_KS:
            for m in DENSE_MS:
                assert lib.plx_gemm_nt_plan(m, n, k, 0) == bm + (1000 if k == 64 else 2000)
    for m, n, k, plan in DENSE_BIG:
        assert lib.plx_gemm_nt_plan(m, n, k, 0) == plan
        assert -(-m // (plan - 1000)) * (n // (128 if plan == 1128 else 64)) == 768
    for mi, (k, s) in enumerate(CONV_MODES):
        seen = set()
        for si, (h, w) in enumerate(CONV_SIZES):
            for cin, cout, nb in conv_cases(mi, si):
                seen.add((cin, cout, nb))
                m = nb * _out(h, k, s) * _out(w, k, s)
                assert lib.plx_gemm_nt_plan(m, cout, k * k * cin, 1) == (2128 if cout % 128 == 0 else 2256)
                assert lib.plx_gemm_nt_plan(nb * h * w, cin, k * k * cout, 1) == (2128 if cin % 128 == 0 else 2256)
        assert len(seen) == 12
    for k, s, nb, cin, cout, h, w, pf, pd in CONV_BIG:
        if pf:
            assert lib.plx_gemm_nt_plan(nb * h * w, cout, 9 * cin, 1) == pf
        if pd:
            assert lib.plx_gemm_nt_plan(nb * h * w, cin, 9 * cout, 1) == pd
    for nb, h, w in STEM_SHAPES:
        assert lib.plx_gemm_nt_plan(nb * _out(h, 7, 2) * _out(w, 7, 2), 64, 256, 1) == 2256
    assert lib.plx_gemm_nt_plan(100, 96, 64, 0) == -1 and lib.plx_gemm_nt_plan(100, 64, 96, 0) == -1
    for (n1, n2), cfg in WGRAD_PAIRS.items():
        assert v2_cfg(n1, n2) == cfg
        m = ragged_m(n1, n2)
        mod = tn_model(m, n1, n2, "v2_64k_atomic")
        assert mod[3] >= 2 and m % mod[2] != 0 and mod[1] == cfg[2]
    cfgs = {v2_cfg(cout, k * k * cin) for cin, cout, k, s in WGRAD_CONVS}
    assert {(1, 3, 2), (2, 1, 4), (4, 1, 2), (2, 2, 2), (1, 1, 8)} <= cfgs


# ---------------------------------------------------------------------------------------------------- the GPU cases
GUARD = 0x7B7B


def _guarded(rows, ld, col0, n, dev, dtype=BF):
    """A [rows][n] view at column col0 of a [rows + 2][ld] buffer filled with a guard pattern, and the buffer."""
    buf = torch.full((rows + 2, ld), GUARD, dtype=torch.int16 if dtype == BF else torch.int32, device=dev).view(dtype)
    return buf[1:rows + 1, col0:col0 + n], buf


def _guards_intact(buf, rows, col0, n):
    raw = buf.view(torch.int16 if buf.dtype == BF else torch.int32).clone()
    raw[1:rows + 1, col0:col0 + n] = GUARD
    return bool((raw == GUARD).all())


def _bnr_args(x, mask, mean, invstd, part, part_ld, blk_off=0, skip_h=0, skip_w=0):
    return _native.GemmBnBwdArgs(x.data_ptr(), mask.data_ptr() if mask is not None else None, mean.data_ptr(),
                                 invstd.data_ptr(), part.data_ptr(), part_ld, blk_off, skip_h, skip_w)


def ctypes_addr(struct):
    return ctypes.addressof(struct)


def _nan32(*shape, dev):
    return torch.full(shape, math.nan, dtype=torch.float32, device=dev)


def _dense_gpu(dev, kind, m, n, k, fam, odev):
    """One dense problem through gemm_nt three ways: forward with stats through strided A and C between guards; the
    data-gradient epilogue with a strided D into a strided C between guards; D under a mask with the BatchNorm partials
    (even-even skip on every other M)."""
    from polyaxon_amd.ops.conv1x1 import gemm_nt

    g = torch.Generator().manual_seed(_seed("dense", m, n, k, kind))
    a, b = _dense_inputs(kind, m, n, k, g)
    d, keep = _addend(kind, (m, n), g), _keep((m, n), g)
    bn = _bn_inputs(kind, m, n, g)
    p, s_abs = ref_nt(a.to(odev), b.to(odev))
    if kind == "exact":
        _assert_exact_range(s_abs)
    case = f"dense-{m}x{n}x{k}"
    nblk = -(-m // _rpb(n))
    abuf = torch.zeros(m, k + 72, dtype=BF, device=dev)
    abuf[:, 64:64 + k] = a.to(dev)
    bd = b.to(dev)
    out, buf = _guarded(m, n + 64, 8, n, dev)
    stats = _nan32(2, nblk, n, dev=dev)
    gemm_nt(abuf[:, 64:64 + k], bd, out, stats=stats.view(-1))
    assert _guards_intact(buf, m, 8, n), case
    judge_nt(kind, fam, case, p, s_abs, k, out, out, stats_got=stats)
    dd = torch.zeros(m, n + 8, dtype=BF, device=dev)
    dd[:, :n] = d.to(dev)
    out, buf = _guarded(m, n + 64, 56, n, dev)
    gemm_nt(abuf[:, 64:64 + k], bd, out, add=dd[:, :n])
    assert _guards_intact(buf, m, 56, n), case
    judge_nt(kind, fam, case + "-add", p, s_abs, k, None, out, d)
    out, buf = _guarded(m, n, 0, n, dev)
    skip = skip_mask(m, 3, 5) if m % 2 else None
    part = _nan32(2, nblk + 1, n, dev=dev)
    xd, mean, invstd = (t.to(dev) for t in bn)
    bits = _pack_bits(keep).to(dev)
    args = _bnr_args(xd, bits, mean, invstd, part, nblk + 1, 1, 3 if skip is not None else 0,
                     5 if skip is not None else 0)
    gemm_nt(a.to(dev), bd, out, add=d.to(dev), add_mask=bits, bnr=args)
    assert _guards_intact(buf, m, 0, n), case
    assert bool(torch.isnan(part[:, 0]).all()), "the partial row before blk_off was written"
    judge_nt(kind, fam, case + "-bwd", p, s_abs, k, None, out, d, keep, bn=bn, part_got=part[:, 1:],
                           skip=skip)


@pytest.mark.gpu
@pytest.mark.parametrize("n", DENSE_NS)
@pytest.mark.parametrize("k", DENSE_KS)
def test_dense_nt(cuda, n, k):
    """gemm_nt at every tile edge in M, both tiles, one / two / odd / many K stages, exact and gauss."""
    assert _lib().plx_gemm_nt_plan(300, n, k, 0) // 1000 == (1 if k == 64 else 2)
    for m in DENSE_MS:
        for kind in KINDS + (("pos",) if m == 300 else ()):       # one sign: sum c = sum |c| in the stats rows
            _dense_gpu(cuda, kind, m, n, k, "dense1" if k == 64 else "dense2", "cpu")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,plan", DENSE_BIG)
def test_dense_nt_single_buffered(cuda, m, n, k, plan):
    """The single-buffered kernels at K > 64 (768 blocks, ragged last tile): forward with stats, and the data-gradient
    epilogue (LATE: accumulators parked in LDS before the epilogue loads) with D, mask and partials."""
    assert _lib().plx_gemm_nt_plan(m, n, k, 0) == plan
    for kind in KINDS + ("pos",):
        _dense_gpu(cuda, kind, m, n, k, "dense1", cuda)
    torch.cuda.synchronize()


def _conv_gpu(dev, kind, cfg, odev, fam_f="conv2", fam_d="conv2", do_f=True, do_d=True):
    """One convolution through plx_conv_fwd (stats) and plx_conv_dgrad: plain, and with D and the BatchNorm partials
    over all launches (a strided 1x1: D == dx in place behind a dense conv1 data gradient that reduces the other
    pixels, BnBwd::skip_w)."""
    lib = _lib()
    k, s, nb, cin, cout, h, w = cfg
    ho, wo = _out(h, k, s), _out(w, k, s)
    g = torch.Generator().manual_seed(_seed("conv", cfg, kind))
    x, wt, dy = _conv_inputs(kind, k, s, nb, cin, cout, h, w, g)
    case = "conv-" + "x".join(map(str, cfg))
    st = _native.current_stream()
    xd, dyd = x.to(dev), dy.to(dev)
    wf, wd = wt.to(dev), wt.permute(2, 1, 0).contiguous().to(dev)
    if do_f:
        m = nb * ho * wo
        assert lib.plx_gemm_nt_plan(m, cout, k * k * cin, 1) // 1000 == (1 if fam_f == "conv1" else 2)
        y, sy = ref_conv_fwd(x.to(odev), wt.to(odev), k, s)
        y, sy = y.view(-1, cout), sy.view(-1, cout)
        if kind == "exact":
            _assert_exact_range(sy)
        out, buf = _guarded(m, cout, 0, cout, dev)
        nblk = -(-m // _rpb(cout))
        stats = _nan32(2, nblk, cout, dev=dev)
        _native.check(lib.plx_conv_fwd(xd.data_ptr(), wf.data_ptr(), out.data_ptr(), nb, h, w, cin, cout, k, s,
                                       stats.data_ptr(), st), "plx_conv_fwd")
        assert _guards_intact(buf, m, 0, cout), case
        judge_nt(kind, fam_f, case, y, sy, k * k * cin, out, out, stats_got=stats)
    if not do_d:
        return
    m = nb * h * w
    assert lib.plx_gemm_nt_plan(m, cin, k * k * cout, 1) // 1000 == (1 if fam_d == "conv1" else 2)
    dx, sx = ref_conv_dgrad(dy.to(odev), wt.to(odev), k, s, h, w)
    dx, sx = dx.view(-1, cin), sx.view(-1, cin)
    if kind == "exact":
        _assert_exact_range(sx)
    s2k1 = s == 2 and k == 1
    written = skip_mask(m, h, w) if s2k1 else torch.ones(m, dtype=torch.bool)
    out, buf = _guarded(m, cin, 0, cin, dev)
    _native.check(lib.plx_conv_dgrad(dyd.data_ptr(), wd.data_ptr(), out.data_ptr(), nb, h, w, cin, cout, k, s, None,
                                     None, st), "plx_conv_dgrad")
    assert _guards_intact(buf, m, 0, cin), case
    raw = out.view(torch.int16).cpu()
    assert bool((raw[~written] == GUARD).all()), case + ": a pixel the strided 1x1 must not write was written"
    wdev = written.to(odev)
    judge_nt(kind, fam_d, case + "-dgrad", dx[wdev], sx[wdev], k * k * cout, None, out.to(odev)[wdev])
    # with D, the mask-free BatchNorm partials and (strided 1x1) the split with a dense data gradient before it
    d = _addend(kind, (m, cin), g)
    bn = _bn_inputs(kind, m, cin, g)
    bx, mean, invstd = (t.to(dev) for t in bn)
    rpb = _rpb(cin)
    rows = dgrad_block_pixels(nb, h, w, k, s, rpb)
    nblk = lib.plx_conv_dgrad_blocks(nb, h, w, cin, cout, k, s)
    assert nblk == len(rows), (nblk, len(rows))
    if not s2k1:
        part = _nan32(2, nblk, cin, dev=dev)
        out, buf = _guarded(m, cin, 0, cin, dev)
        args = _bnr_args(bx, None, mean, invstd, part, nblk)
        dd = d.to(dev)
        _native.check(lib.plx_conv_dgrad(dyd.data_ptr(), wd.data_ptr(), out.data_ptr(), nb, h, w, cin, cout, k, s,
                                         dd.data_ptr(), ctypes_addr(args), st), "plx_conv_dgrad")
        assert _guards_intact(buf, m, 0, cin), case
        judge_nt(kind, fam_d, case + "-dgrad-bn", dx, sx, k * k * cout, None, out, d, bn=bn,
                               part_got=part, block_rows=rows)
        return
    # conv1's dense data gradient dx1 (K = 64) reduces every pixel but the even-even ones into rows [0, nblk1); the
    # strided 1x1 then adds its product to the even-even pixels of dx1 in place and reduces them into the rows after
    from polyaxon_amd.ops.conv1x1 import gemm_nt
    a1, b1 = _dense_inputs(kind, m, cin, 64, g)
    nblk1 = -(-m // rpb)
    part = _nan32(2, nblk1 + nblk, cin, dev=dev)
    out, buf = _guarded(m, cin, 0, cin, dev)
    gemm_nt(a1.to(dev), b1.to(dev), out, bnr=_bnr_args(bx, None, mean, invstd, part, nblk1 + nblk, 0, h, w))
    dx1 = out.clone()
    p1, s1 = ref_nt(a1.to(odev), b1.to(odev))
    judge_nt(kind, "dense1", case + "-conv1", p1, s1, 64, None, dx1, bn=bn, part_got=part[:, :nblk1],
                           skip=skip_mask(m, h, w))
    args = _bnr_args(bx, None, mean, invstd, part, nblk1 + nblk, nblk1)
    _native.check(lib.plx_conv_dgrad(dyd.data_ptr(), wd.data_ptr(), out.data_ptr(), nb, h, w, cin, cout, k, s,
                                     out.data_ptr(), ctypes_addr(args), st), "plx_conv_dgrad")
    assert _guards_intact(buf, m, 0, cin), case
    assert torch.equal(out.cpu()[~written].view(torch.int16), dx1.cpu()[~written].view(torch.int16)), \
        case + ": D == dx in place must leave the other pixels alone"
    judge_nt(kind, fam_d, case + "-dgrad-inplace", dx[wdev], sx[wdev], k * k * cout, None,
                           out.to(odev)[wdev], dx1.to(odev)[wdev])
    judge_nt(kind, fam_d, case + "-dgrad-rest", dx, sx, k * k * cout, None, out, bn=bn,
                           part_got=part[:, nblk1:], block_rows=rows, judge_c=False)


@pytest.mark.gpu
@pytest.mark.parametrize("size_i", range(len(CONV_SIZES)), ids=[f"{h}x{w}" for h, w in CONV_SIZES])
@pytest.mark.parametrize("mode_i", range(len(CONV_MODES)), ids=[f"k{k}s{s}" for k, s in CONV_MODES])
def test_conv_geometry_edges(cuda, mode_i, size_i):
    """plx_conv_fwd / plx_conv_dgrad at 1-pixel sides (the d == 1 branch of the magic divisors; at stride 2 the empty
    parity classes), images smaller than a tile, tile boundaries inside an image row, and a side above 255."""
    k, s = CONV_MODES[mode_i]
    h, w = CONV_SIZES[size_i]
    for cin, cout, nb in conv_cases(mode_i, size_i):
        for kind in KINDS:
            _conv_gpu(cuda, kind, (k, s, nb, cin, cout, h, w), "cpu")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONV_BIG, ids=["fwd128", "dgrad128", "fwd256", "dgrad256"])
def test_conv_single_buffered(cuda, cfg):
    """The gathered single-buffered kernels (>= 768 blocks) on both tiles: forward with stats, and the data gradient
    with D and partials (LATE)."""
    *geo, pf, pd = cfg
    for kind in KINDS:
        _conv_gpu(cuda, kind, tuple(geo), cuda, "conv1", "conv1", do_f=pf is not None, do_d=pd is not None)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("k,s,shape,cout", [(3, 1, (3, 128, 9, 11), 128), (3, 2, (2, 64, 7, 9), 192),
                                            (1, 2, (3, 64, 5, 17), 128)])
def test_convkxk_autograd(cuda, k, s, shape, cout):
    """The same oracle through ops.conv.conv_k's autograd path (weight prep, stats hand-off, the zeroed dx of a strided
    1x1, the channels_last weight gradient view): y, stats, dx and dW."""
    from polyaxon_amd.ops.conv import ConvKxK, conv_k, supported

    nb, cin, h, w = shape
    for kind in KINDS:
        g = torch.Generator().manual_seed(_seed("module", k, s, shape, cout, kind))
        x, wt, dy = _conv_inputs(kind, k, s, nb, cin, cout, h, w, g)
        conv = ConvKxK(cin, cout, k, s).to(cuda)
        conv.weight.data = wt.float().view(cout, k, k, cin).permute(0, 3, 1, 2).to(cuda)
        xa = x.to(cuda).permute(0, 3, 1, 2).requires_grad_()
        assert supported(xa, conv)
        with _Hooks("v2_64k_atomic"):
            y = conv_k(xa, conv.weight, s, with_stats=True)
            stats, nblk = y._plx_channel_stats
            y.backward(dy.to(cuda).permute(0, 3, 1, 2))
            torch.cuda.synchronize()
        case = f"module-k{k}s{s}-" + "x".join(map(str, shape)) + f"-{cout}"
        yr, sy = ref_conv_fwd(x, wt, k, s)
        q = y.detach().permute(0, 2, 3, 1).reshape(-1, cout).cpu()
        judge_nt(kind, "conv2", case, yr.view(-1, cout), sy.view(-1, cout), k * k * cin, q, q,
                 stats_got=stats.view(2, nblk, cout).cpu())
        dx, sx = ref_conv_dgrad(dy, wt, k, s, h, w)              # a strided 1x1: exact zeros off the even-even pixels
        got = xa.grad.permute(0, 2, 3, 1).reshape(-1, cin).cpu()
        judge_nt(kind, "conv2", case + "-dgrad", dx.view(-1, cin), sx.view(-1, cin), k * k * cout, None, got)
        dw, sw = ref_conv_wgrad(dy, x, k, s)
        mod = tn_model(dy.numel() // cout, cout, k * k * cin, "v2_64k_atomic", _cus(cuda))
        got = conv.weight.grad.permute(0, 2, 3, 1).reshape(cout, -1)
        check(kind, mod[0], case, "dw", got, dw.view(cout, -1), bound_wgrad(sw.view(cout, -1), 0.0, mod, False))


class _Hooks:
    """The weight-gradient kernel selection of one variant; the defaults again on exit."""

    def __init__(self, hook, stem=0):
        self.hook, self.stem = hook, stem

    def __enter__(self):
        lib = _lib()
        on, kb, atomic, c64 = HOOKS[self.hook]
        lib.plx_set_tn_v2(on, kb)
        lib.plx_set_tn_atomic(atomic)
        lib.plx_set_tn2_c64(c64)
        lib.plx_set_tn2_stem(self.stem)

    def __exit__(self, *exc):
        lib = _lib()
        lib.plx_set_tn_v2(1, 64)
        lib.plx_set_tn2_stem(0)
        lib.plx_set_tn2_c64(1)
        lib.plx_set_tn_atomic(int(os.environ.get("PLX_WGRAD_ATOMIC", "1")))


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", list(WGRAD_PAIRS), ids=[f"{a}x{b}" for a, b in WGRAD_PAIRS])
def test_wgrad_dense(cuda, n1, n2):
    """gemm_tn on every v2 configuration under every kernel variant: M of less than a step, a step +- 1, 4 steps of the
    block +- 1, and the smallest M with >= 2 slices and a ragged last one; the product written over garbage, and
    accumulated into an integer / gauss base, through ldc > N2 with the padding columns untouched."""
    from polyaxon_amd.ops.conv1x1 import gemm_tn

    cus = _cus(cuda)
    ms = wgrad_ms(n1, n2) if cus == CUS else [1, 31, 32, 33, ragged_m(n1, n2, cus=cus)]
    for kind in KINDS_W:
        for m in ms:
            g = torch.Generator().manual_seed(_seed("wgrad", m, n1, n2, kind))
            a, b = _acts(kind, (m, n1), g), _acts(kind, (m, n2), g)
            base = _addend(kind, (n1, n2), g).float()
            ref = a.to(F64).t() @ b.to(F64)
            s_abs = a.to(F64).abs().t() @ b.to(F64).abs()
            if kind == "exact":
                _assert_exact_range(s_abs + base.abs())
            ad, bd = a.to(cuda), b.to(cuda)
            for hook in HOOKS:
                mod = tn_model(m, n1, n2, hook, cus)
                for accumulate in (False, True):
                    out, buf = _guarded(n1, n2 + 64, 32, n2, cuda, torch.float32)
                    out.copy_(base if accumulate else torch.full_like(base, math.nan))
                    with _Hooks(hook):
                        gemm_tn(ad, bd, out=out, accumulate=accumulate)
                    torch.cuda.synchronize()
                    assert _guards_intact(buf, n1, 32, n2), (m, hook)
                    b64 = base.to(F64) if accumulate else torch.zeros_like(ref)
                    check(kind, mod[0], f"tn-{m}x{n1}x{n2}-{hook}-acc{int(accumulate)}", "dw", out, ref + b64,
                              bound_wgrad(s_abs, b64.abs(), mod, accumulate))


@pytest.mark.gpu
@pytest.mark.parametrize("hook", list(HOOKS))
def test_wgrad_conv(cuda, hook):
    """plx_conv_wgrad's gathered forms (3x3 at stride 1 and 2, 1x1 at stride 2) under each kernel variant, on an image
    batch of one slice and one of several."""
    lib = _lib()
    cus = _cus(cuda)
    st = _native.current_stream()
    for cin, cout, k, s in WGRAD_CONVS:
        for nb, h, w in WGRAD_CONV_SHAPES:
            for kind in KINDS:
                g = torch.Generator().manual_seed(_seed("wconv", cin, cout, k, s, nb, h, w, kind))
                x, _, dy = _conv_inputs(kind, k, s, nb, cin, cout, h, w, g)
                m = dy.shape[0] * dy.shape[1] * dy.shape[2]
                dw, sw = ref_conv_wgrad(dy, x, k, s)
                dw, sw = dw.view(cout, -1), sw.view(cout, -1)
                base = _addend(kind, tuple(dw.shape), g).float()
                if kind == "exact":
                    _assert_exact_range(sw + base.abs())
                mod = tn_model(m, cout, k * k * cin, hook, cus)
                xd, dyd = x.to(cuda), dy.to(cuda)
                ws = torch.empty(lib.plx_conv_wgrad_workspace(nb, h, w, cin, cout, k, s, cus), dtype=torch.float32,
                                 device=cuda)
                for accumulate in (0, 1):
                    out, buf = _guarded(cout, k * k * cin, 0, k * k * cin, cuda, torch.float32)
                    out.copy_(base if accumulate else torch.full_like(base, math.nan))
                    with _Hooks(hook):
                        _native.check(lib.plx_conv_wgrad(dyd.data_ptr(), xd.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                         nb, h, w, cin, cout, k, s, cus, accumulate, st),
                                      "plx_conv_wgrad")
                    torch.cuda.synchronize()
                    assert _guards_intact(buf, cout, 0, k * k * cin), (cin, cout, k, s)
                    b64 = base.to(F64) if accumulate else torch.zeros_like(dw)
                    check(kind, mod[0], f"wconv-{cin}x{cout}k{k}s{s}-{nb}x{h}x{w}-{hook}-acc{accumulate}", "dw",
                              out, dw + b64, bound_wgrad(sw, b64.abs(), mod, bool(accumulate)))


@pytest.mark.gpu
@pytest.mark.parametrize("stem_mode", [0, 1, 2])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=["x".join(map(str, s)) for s in STEM_SHAPES])
def test_stem(cuda, shape, stem_mode):
    """StemConv forward with stats and its weight gradient under the three plx_set_tn2_stem kernels."""
    from polyaxon_amd.ops.stem import StemConv, stem_conv_supported

    nb, h, w = shape
    for kind in KINDS:
        g = torch.Generator().manual_seed(_seed("stem", shape, kind))
        x, wt, dy = _conv_inputs(kind, 7, 2, nb, 3, 64, h, w, g)
        y, sy = ref_conv_fwd(x, wt, 7, 2)
        y, sy = y.view(-1, 64), sy.view(-1, 64)
        dw, sw = ref_conv_wgrad(dy, x, 7, 2)
        if kind == "exact":
            _assert_exact_range(sy, sw)
        conv = StemConv().to(cuda)
        conv.weight.data.copy_(wt.float().view(64, 7, 7, 3).permute(0, 3, 1, 2))
        xin = x.to(cuda).permute(0, 3, 1, 2)                      # NCHW view of NHWC memory: channels_last
        assert stem_conv_supported(xin, conv)
        case = f"stem-{nb}x{h}x{w}-mode{stem_mode}"
        with _Hooks("v2_64k_atomic", stem_mode):
            out = conv(xin)
            stats, nblk = out._plx_channel_stats
            out.backward(dy.to(cuda).permute(0, 3, 1, 2))
            torch.cuda.synchronize()
        m = y.shape[0]
        assert nblk == -(-m // 256)
        q = out.detach().permute(0, 2, 3, 1).reshape(-1, 64)
        judge_nt(kind, "stem", case, y, sy, 147, q.cpu(), q.cpu(), stats_got=stats.view(2, nblk, 64).cpu())
        got = conv.weight.grad.permute(0, 2, 3, 1).reshape(64, 49, 3)
        check(kind, "stem", case, "dw", got, dw, bound_stem_dw(sw, m))


@pytest.mark.gpu
def test_argument_validation_returns_without_a_launch(cuda):
    """The -1 returns of the argument checks: the output keeps its guard pattern, no kernel ran."""
    lib = _lib()
    st = _native.current_stream()
    m = 64
    a = torch.zeros(m, 128, dtype=BF, device=cuda)
    b = torch.zeros(128, 128, dtype=BF, device=cuda)
    d = torch.zeros(m, 128, dtype=BF, device=cuda)
    bits = torch.zeros(m * 128 // 8, dtype=torch.uint8, device=cuda)
    f = torch.zeros(4 * 128, device=cuda)
    out, buf = _guarded(m, 192, 0, 192, cuda)

    def nt(n, k, ldc, dptr, mptr, bnr):
        return lib.plx_gemm_nt(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, 128, 128, ldc, None, dptr, 128,
                               mptr, bnr, st)
    assert nt(96, 64, 192, None, None, None) == -1               # N % 64
    assert nt(64, 96, 192, None, None, None) == -1               # K % 64
    assert nt(128, 64, 192, None, bits.data_ptr(), None) == -1   # dmask without D
    args = _bnr_args(d, None, f, f, f, 1)
    assert nt(128, 64, 192, None, None, ctypes_addr(args)) == -1  # bnr with ldc != N
    x = torch.zeros(1, 4, 4, 64, dtype=BF, device=cuda)
    dy = torch.zeros(1, 2, 2, 64, dtype=BF, device=cuda)
    wd = torch.zeros(64, 1, 64, dtype=BF, device=cuda)
    dx, xbuf = _guarded(16, 64, 0, 64, cuda)
    args = _bnr_args(x, None, f, f, f, 2, 0)
    assert lib.plx_conv_dgrad(dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), 1, 4, 4, 64, 64, 1, 2, None,
                              ctypes_addr(args), st) == -1       # K = 1, S = 2 with blk_off == 0
    torch.cuda.synchronize()
    raw, xraw = buf.view(torch.int16), xbuf.view(torch.int16)
    assert bool((raw == GUARD).all()) and bool((xraw == GUARD).all())
