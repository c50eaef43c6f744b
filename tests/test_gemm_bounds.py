"""The 256x256 LM GEMM (csrc/gemm256.hip) on exact integer data and against derived per-element bounds.

tests/test_gpu_gemm.py judges these kernels by max |out - ref| <= 1.5e-2 max |ref| + 1e-3 (fused GELU: rtol = atol =
1e-2).  Here every output element is compared with an fp64 reference of the same operation (A and B are bf16, so an
fp64 matmul of them is exact to 2^-53 of sum |a b|), through the C entry points plx_gemm256_exv / plx_gemm256_sk
(leading dimensions, variant, workspace and tickets of the test's own) and, for a few cases, through ops/gemm.py.

Data
  exact   A in {-1, 0, 1} (~3/4 zeros) times a power of two, B on the grid k / 64, |k| <= 128 (-2 .. 2, but finer,
          so that the outputs carry more than 8 significant bits: the generator asserts that >= 5 % of them are not
          bf16 values and the final rounding is exercised), bias and C0 small integers, alpha in {1, 0.5, -2}.  The
          generator asserts (|alpha| sum |a b| + |bias| + |C0|) / unit < 2^24 for the common grid `unit` of all terms,
          so every fp32 partial sum is exact in any order -- K-tiles, slabs, stream-K pieces, the read-modify-write of
          accumulate -- and the bf16 output must equal torch's round-to-nearest-even of the fp64 value bit for bit.
  gauss   randn rounded to bf16;  pos: its absolute value (partial sums as large as the S the bound is written in).
          Statistic max |got - ref| / bound, asserted <= 1; where the bound is 0 the element must be exact.

The bound.  U = 2^-8 (one bf16 store), E = 2^-23 per addition inside an MFMA accumulation chain (the guides do not
state the bf16 MFMA's internal rounding; 2^-23 holds for round-to-nearest and truncation in any order), EV = 2^-24 per
VALU fp32 operation, gamma(x) = x / (1 - x), S = sum |a_k b_k|, c = 2 (the alpha multiply and the bias add):
  one pass    gemm256_tile :393-:409 / gemm256w4_kernel :934-:953 add all K products into one fp32 accumulator, two
              MFMA steps of 32 per K-tile; store_pair :265-:266 `a * alpha + bias`, pack_bf16x2 :91:
                  U |ref| + (1 + U) gamma(K E + c EV) (|alpha| S + |bias|)
  accumulate  store_pair :256 `alpha * a + C0` (gemm256_reduce :1015-:1025 adds C0 last): |C0| inside the
              parentheses, one more EV.
  split-K     a slab holds the K of one split (kt_per_split * 64, plx_gemm256_kt_per_split; kernel :602-:603, :621);
              gemm256_reduce :1003-:1007 adds `splits` slabs in sequence, then alpha :1008, bias :1011:
                  gamma(kt_per_split 64 E + (splits + c) EV)      -- not the whole K
  stream-K    a piece holds its own K-tiles (gemm256_sk_kernel :673-:680, cut at multiples of ipb); the last arriver
              adds the np pieces of its tile in workgroup order from zero :754-:774 (np - 1 roundings), then
              store_pair: gamma(longest piece 64 E + (np - 1 + c) EV), per tile (tile_of :74).
  gelu_out    store_pair :287 / gemm256_reduce :1034: gelu_tanh(bf16_round(v)), against fp64 gelu_tanh of the bf16 C
              the kernel itself stored: U |gelu| + (1 + U) err_gelu(c), err_gelu below.
  gelu_h      store_pair :269: bf16_round(v) * gelu_tanh_grad(h).  On exact data D = bf16(alpha A.B) is known exactly:
              U |D g| + (1 + U) |D| (err_grad(h) + EV |g|).  On gauss data D may round to the neighbouring bf16 value:
              b_D = U |dA| + (1 + U) chain, and the error before the store is b_D |g| + (|dA| + b_D)(err_grad + EV |g|).
  formulas    (:196-:212) x = 2 k0 (h + k1 h^3): (k1 h) h, the fmaf, the k0 multiply, the constants k0 and k1 and,
              inside __expf, the log2(e) multiply and its constant: 8 EV |x| in the exponent, so e = exp(x) is within
              eta = expm1(8 EV |x|) + C_EXP 2^-23 relative; r = rcp(1 + e): dr = r (2 EV + C_RCP 2^-23) + 2 eta r(1 - r)
              (+ 2^-120 for the flush of e outside fp32's range).
              gelu: s = 2 - 2 r, ds = 2 dr + EV s, err_gelu = |h / 2| ds + EV |gelu|.  At h << 0 (s -> 0, 2 r -> 2) the
              cancellation leaves the absolute term |h| (EV + C_RCP 2^-23): it is what holds the check at h ~ -4
              (gelu ~ -7e-5) and in the saturated tails.
              grad: t = 1 - 2 r, dt = 2 dr + EV |t|; 1 + t: dt + EV (1 + t); 1 - t t: d2 = 2 |t| dt + dt^2 + EV t^2 +
              EV (1 - t^2) -- the cancellation at large |h|, multiplied below by |h / 2| k0 (1 + 3 k1 h^2);
              q = (h / 2)(1 - t^2) k0 poly: poly within 4 EV, the k0 constant, three multiplies; then the last fmaf:
              err_grad = (dt + EV (1 + t)) / 2 + |h / 2 k0 poly| d2 + 8 EV |q| + EV |g|.
              (Where the compiler fuses 2 - 2 r or (h / 2)(1 - t t) into one fma there is one rounding fewer.)
              Neither guide states the accuracy of v_exp_f32 / v_rcp_f32: C_EXP = C_RCP = 1 ulp is an ASSUMPTION
              (cap 4).  Measured at C_EXP = C_RCP = 1: the `formula` rows of the table; not raised.

gelu_tanh_grad at |h| >= 2^64 (~1.8e19): h * h overflowed, 1 - t t is 0 and `0 * inf` made the derivative NaN (7 of 8
elements of test_gelu_grad_at_huge_h on an MI355X, in both copies of the formula, gemm256.hip and lm_kernels.hip).
Both now cap the square below the overflow; the test holds them to the true derivative, exactly 0 or 1.

Layout: data and oracle; the bounds; an fp32 emulation of each dataflow with the CPU tests (bit-exact on exact data,
inside the bound on gauss / pos, injected defects outside, the old tolerance's verdicts on record, every listed case
at the plan it is listed for); then the GPU cases.

Largest measured ratio per family on an MI355X (GEMM_RATIO lines; the emulation's over the CPU-sized cases in
brackets; every exact comparison was bit-equal):

    family      output     MI355X   emulation
    8-wave      c          0.994    (0.994)
    4-wave      c          0.994    (the same dataflow)
    split-K     c          0.945    (0.928)
    stream-K    c          0.988    (0.988)
    gelu_out    g          0.986    (0.986)
    gelu_out    formula    0.245    (0.245)     C_EXP = C_RCP = 1
    gelu_h      dh         0.996    (0.993)
    gelu_h      formula    0.880    (0.858)     C_EXP = C_RCP = 1; 0.243 on exact data, where D is known

Every bf16 output sits at the bf16 rounding itself (U |ref| is reached when the fp32 value lies next to a rounding
boundary just above a power of two); no family is far below its bound, the lowest is split-K at 0.945.
`formula` is the part of an error that the final rounding cannot explain (formula_need: |got - ref| minus half an ulp
of the stored value) over the formula's allowance alone, so it isolates the term that carries the two assumed
constants: both epilogues use a quarter of it at 1 ulp each (on gauss data gelu_h's allowance also carries the
data gradient's own rounding, which dominates), so the constants stay at 1.  It is a quarter and not more because the
allowance charges every operation its worst case at once and the two instructions a whole ulp; it was left there:
halving the constants would need a statement about v_exp_f32 / v_rcp_f32 that neither guide makes.
"""
import ctypes
import math
import zlib

import pytest
import torch

from polyaxon_amd.ops import _native

U = 2.0 ** -8             # bf16 round-to-nearest unit roundoff
E = 2.0 ** -23            # per addition of an MFMA accumulation chain
EV = 2.0 ** -24           # per VALU fp32 operation
C_EXP = 1.0               # ulps (2^-23 relative) charged to v_exp_f32: an assumption, see the docstring
C_RCP = 1.0               # the same for v_rcp_f32
BF = torch.bfloat16
F64 = torch.float64
K0 = math.sqrt(2.0 / math.pi)
K1 = 0.044715
TILE, BK = 256, 64
QB = 2.0 ** -6            # grid of the exact B entries
CUS = 256                 # MI355X; without a device the planner assumes it
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]
KINDS = ("exact", "gauss")


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _gamma(x):
    return x / (1 - x)


def _lib():
    return _native.lib("plx_gemm")


def _gen(dev, *key):
    return torch.Generator(device=dev).manual_seed(zlib.crc32(repr(key).encode()))


# --------------------------------------------------------------------------------------------------------- the data
def _matrix(kind, which, shape, g, dev):
    if kind == "gauss":
        return torch.randn(shape, generator=g, device=dev).to(BF)
    if kind == "pos":
        return torch.randn(shape, generator=g, device=dev).abs().to(BF)
    if which == "a":
        r = torch.randint(0, 8, shape, generator=g, device=dev)
        return torch.where(r == 0, 1.0, torch.where(r == 1, -1.0, 0.0)).to(BF)
    return (torch.randint(-128, 129, shape, generator=g, device=dev).float() * QB).to(BF)


class Problem:
    """A [M][K], B [N][K] (logical, bf16), P = A . B^T and S = |A| . |B|^T in fp64; shared by the tests of a shape."""

    def __init__(self, dev, kind, M, N, K, scale):
        g = _gen(dev, "gemm256", kind, M, N, K)
        self.kind, self.M, self.N, self.K, self.scale, self.dev = kind, M, N, K, scale, dev
        self.a = (_matrix(kind, "a", (M, K), g, dev).float() * scale).to(BF)
        self.b = _matrix(kind, "b", (N, K), g, dev)
        a64, b64 = self.a.to(F64), self.b.to(F64)
        self.P = a64 @ b64.t()
        self.S = a64.abs() @ b64.abs().t()

    def extras(self, what, bias_mode=None):
        """bias (fp32 [N]), C0 (bf16 [M][N]) and h (bf16 [M][N]) of the problem, by name."""
        g = _gen(self.dev, "extras", what, self.kind, self.M, self.N)
        if what == "bias":
            if self.kind == "exact":
                v = torch.randint(-4, 5, (self.N,), generator=g, device=self.dev).float()
            else:
                v = 2.0 * torch.randn(self.N, generator=g, device=self.dev)
            if bias_mode == "gelu":      # columns n % 8 = 1, 2, 3, 4 shift the output to ~ -4, +34, -34, 0 (integers)
                n = torch.arange(self.N, device=self.dev) % 8
                for j, val in ((1, -4.0), (2, 34.0), (3, -34.0), (4, 0.0)):
                    v = torch.where(n == j, torch.full_like(v, val), v)
            return v
        if what == "c0":
            if self.kind == "exact":
                return torch.randint(-4, 5, (self.M, self.N), generator=g, device=self.dev).float().to(BF)
            return (3.0 * torch.randn(self.M, self.N, generator=g, device=self.dev)).to(BF)
        assert what == "h"               # mostly N(0, 2^2); every 8th column group at 0, ~ -4, and +-(30 .. 40)
        h = 2.0 * torch.randn(self.M, self.N, generator=g, device=self.dev)
        sel = torch.randint(0, 16, (self.M, self.N), generator=g, device=self.dev)
        far = (30.0 + 10.0 * torch.rand(self.M, self.N, generator=g, device=self.dev))
        h = torch.where(sel == 0, torch.zeros_like(h), h)
        h = torch.where(sel == 1, -4.0 + 0.25 * h, h)
        h = torch.where(sel == 2, far, h)
        h = torch.where(sel == 3, -far, h)
        return h.to(BF)


_PROBLEMS = {}


def problem(dev, kind, M, N, K, scale=1.0):
    key = (str(dev), kind, M, N, K, scale)
    if key not in _PROBLEMS:
        if len(_PROBLEMS) >= 12 or M * N > 2 ** 22:
            _PROBLEMS.clear()
        _PROBLEMS[key] = Problem(dev, kind, M, N, K, scale)
    return _PROBLEMS[key]


def gelu_scale(kind, K):
    """Power of two that brings the products' spread to ~4, so a GELU epilogue sees h between its two tails."""
    std = math.sqrt(K) * (0.6 if kind == "exact" else 1.0)
    return 2.0 ** -max(0, round(math.log2(std / 4.0)))


def rne(x):
    return x.float().to(BF).to(F64)


def reference(p, alpha, bias, c0):
    """(ref, mag): alpha A.B + bias + C0 in fp64 and |alpha| S + |bias| + |C0|; asserts the exact kind's promises."""
    ref, mag = alpha * p.P, abs(alpha) * p.S
    if bias is not None:
        ref, mag = ref + bias.to(F64), mag + bias.to(F64).abs()
    if c0 is not None:
        ref, mag = ref + c0.to(F64), mag + c0.to(F64).abs()
    if p.kind == "exact":
        unit = p.scale * QB * min(1.0, abs(alpha))
        assert unit <= 1.0 and float(mag.max()) / unit < 2 ** 24, (float(mag.max()), unit)
        share = float((rne(ref) != ref).double().mean())
        assert share >= 0.05, f"only {share:.3f} of the exact outputs need the final rounding"
    return ref, mag


# ----------------------------------------------------------------------------------------------------- the formulas
def gelu64(h):
    return 0.5 * h * (1 + torch.tanh(K0 * (h + K1 * h ** 3)))


def gelu_grad64(h):
    t = torch.tanh(K0 * (h + K1 * h ** 3))
    return 0.5 * (1 + t) + 0.5 * h * (1 - t * t) * K0 * (1 + 3 * K1 * h * h)


def _rcp_chain(h):
    """r = 1 / (1 + e^x), x = 2 k0 (h + k1 h^3), its error dr, and e r (= 1 - r without the cancellation)."""
    x = 2 * K0 * (h + K1 * h ** 3)
    e = torch.exp(x.clamp(-700.0, 700.0))
    r = 1 / (1 + e)
    eta = torch.expm1(8 * EV * x.abs()).clamp(max=0.5) + C_EXP * 2.0 ** -23
    dr = r * (2 * EV + C_RCP * 2.0 ** -23) + 2 * eta * r * (e * r) + 2.0 ** -120
    return r, dr, e * r


SLOP = 1 + 2.0 ** -16     # the second-order terms of the sums below


def gelu_err(h):
    """fp32 error of gelu_tanh(h) (:196) at an fp32 h, before the bf16 store."""
    r, dr, er = _rcp_chain(h)
    s = 2 * er
    return SLOP * ((0.5 * h).abs() * (2 * dr + EV * s) + EV * gelu64(h).abs())


def gelu_grad_err(h):
    """fp32 error of gelu_tanh_grad(h) (:205)."""
    r, dr, er = _rcp_chain(h)
    t = 1 - 2 * r
    dt = 2 * dr + EV * t.abs()
    one_t = 2 * er
    s2 = 4 * er * r                                               # 1 - t^2
    d2 = 2 * t.abs() * dt + dt * dt + EV * t * t + EV * s2
    poly = 1 + 3 * K1 * h * h
    lead = (0.5 * h).abs() * K0 * poly
    q = lead * s2
    return SLOP * (0.5 * (dt + EV * one_t) + lead * d2 + 8 * EV * q + EV * gelu_grad64(h).abs())


# ------------------------------------------------------------------------------------------------------- the plans
def tile_of(i, ntm, ntn, group):
    """gemm256.hip tile_of (:74)."""
    per = group * ntn
    first = (i // per) * group
    gs = min(ntm - first, group)
    r = i - (i // per) * per
    return first + r % gs, r // gs


def split_plan(M, N, K):
    """(kt_per_split, [K-tiles of each split])."""
    lib = _lib()
    kps, ns, nk = lib.plx_gemm256_kt_per_split(M, N, K), lib.plx_gemm256_splits(M, N, K), K // BK
    lens = [min(kps, nk - s * kps) for s in range(ns)]
    assert sum(lens) == nk and min(lens) >= 1 and ns == -(-nk // kps), (kps, ns, nk)
    return kps, lens


def sk_plan(M, N, K):
    """(G, sk_tiles, ipb) of plx_gemm256_sk_plan under the current sk_force."""
    t, i = ctypes.c_int(0), ctypes.c_int(0)
    g = _lib().plx_gemm256_sk_plan(M, N, K, ctypes.byref(t), ctypes.byref(i))
    return g, t.value, i.value


def sk_pieces(t, nk, ipb):
    """K-tile ranges of stream-K tile t: the flattened iteration space is cut at multiples of ipb (:668-:679)."""
    i, end, out = t * nk, (t + 1) * nk, []
    while i < end:
        j = min(end, (i // ipb + 1) * ipb)
        out.append((i - t * nk, j - t * nk))
        i = j
    return out


def chain_of(path, M, N, K, group, dev):
    """(products in the longest MFMA chain, VALU additions that join the chains): scalars, or [M][N] for stream-K."""
    if path == "exv":
        kps, lens = split_plan(M, N, K)
        return (K, 0) if len(lens) == 1 else (kps * BK, len(lens))
    g, skt, ipb = sk_plan(M, N, K)
    ntm, ntn, nk = M // TILE, N // TILE, K // BK
    ck = torch.full((ntm, ntn), float(K), dtype=F64)
    ad = torch.zeros(ntm, ntn, dtype=F64)
    for t in range(skt):
        pcs = sk_pieces(t, nk, ipb)
        tm, tn = tile_of(t, ntm, ntn, group)
        ck[tm, tn] = BK * max(e - b for b, e in pcs)
        ad[tm, tn] = len(pcs) - 1
    big = lambda v: v.to(dev).repeat_interleave(TILE, 0).repeat_interleave(TILE, 1)
    return big(ck), big(ad)


def bound_c(ref, mag, chain, accumulate):
    ck, adds = chain
    return U * ref.abs() + (1 + U) * _gamma(ck * E + (adds + 2 + (1 if accumulate else 0)) * EV) * mag


# ------------------------------------------------------------------------------------------------------ the verdicts
def ratio(got, ref, bound):
    err = (got.to(F64) - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return r


def where(bad, limit=4):
    """The first bad elements as (tile, 128x64 wave block of the 8-wave kernel, column within the 32-column pair)."""
    out = []
    for m, n in bad.nonzero()[:limit].tolist():
        out.append(f"[{m}][{n}] tile ({m // TILE},{n // TILE}) wave block ({m % TILE // 128},{n % TILE // 64}) "
                   f"pair column {n % 32}")
    return "; ".join(out)


def ktile_diagnosis(p, alpha, ref, got, bad, limit=4):
    """Exact data: is a wrong value the reference with one K-tile removed or doubled?"""
    notes = []
    for m, n in bad.nonzero()[:limit].tolist():
        per = (p.a[m].to(F64) * p.b[n].to(F64)).view(-1, BK).sum(1) * alpha
        g = float(got[m, n])
        hit = [f"K-tile {k} removed" for k in range(per.numel()) if float(rne(ref[m, n] - per[k])) == g]
        hit += [f"K-tile {k} doubled" for k in range(per.numel()) if float(rne(ref[m, n] + per[k])) == g]
        notes.append(f"[{m}][{n}] got {g} want {float(rne(ref[m, n]))}: {', '.join(hit[:3]) or 'no single K-tile'}")
    return "; ".join(notes)


def formula_need(got, ref):
    """The least fp32 error that explains a stored bf16 value: round-to-nearest moved the fp32 result by at most half
    an ulp of what it stored (the larger half at a power of two), the rest is the formula's own."""
    g = got.to(F64)
    _, ex = torch.frexp(g.abs().clamp_min(2.0 ** -126))
    need = ((g - ref).abs() - torch.ldexp(torch.ones_like(g), ex - 9)).clamp_min(0)
    return torch.where(torch.isnan(need), torch.full_like(need, math.inf), need)


RATIOS = {}               # (family, output) -> the largest ratio seen in this process


def check(kind, family, case, name, got, ref, bound, p=None, alpha=1.0):
    """exact: bit equality with round-to-nearest-even of the reference; else ratio <= 1, printed first."""
    if kind == "exact":
        want = rne(ref)
        bad = got.to(F64) != want                                   # NaN (an unwritten element) differs
        n = int(bad.sum())
        assert n == 0, f"{family} {case} {name}: {n} of {want.numel()} differ on exact data: {where(bad)}" + \
                       (f" | {ktile_diagnosis(p, alpha, ref, got, bad)}" if p is not None else "")
        return 0.0
    r = ratio(got, ref, bound)
    top = float(r.max())
    print(f"GEMM_RATIO {family} {case}{'' if kind == 'bound' else '-' + kind} {name} {top:.4f}")
    RATIOS[family, name] = max(RATIOS.get((family, name), 0.0), top)
    assert top <= 1.0, f"{family} {case} {name}: ratio {top} at {where(r > 1.0)}"
    return top


def judge(p, fam, case, alpha, bias, c0, chain, got_c, got_g=None, h=None, prefix=""):
    """C (or, with h, the fused GELU backward stored in its place) and the GELU output of one launch."""
    fam = prefix + fam
    accumulate = c0 is not None
    ref, mag = reference(p, alpha, bias, c0)
    bc = bound_c(ref, mag, chain, accumulate)
    if h is None:
        check(p.kind, fam, case, "c", got_c, ref, bc, p, alpha)
    else:
        h64 = h.to(F64)
        g, eg = gelu_grad64(h64), gelu_grad_err(h64)
        if p.kind == "exact":
            d, bd = rne(ref), torch.zeros_like(ref)
        else:
            d, bd = ref, bc
        val = d * g
        e1 = bd * g.abs() + (d.abs() + bd) * (eg + EV * g.abs())
        check("bound", prefix + "gelu_h", f"{case}-{p.kind}", "dh", got_c, val, U * val.abs() + (1 + U) * e1)
        check("bound", prefix + "gelu_h", f"{case}-{p.kind}", "formula", val + formula_need(got_c, val), val, e1)
    if got_g is not None:
        c64 = got_c.to(F64)
        gref = gelu64(c64)
        if bias is not None:                                       # the generator's promise: both tails, ~ -4, and 0
            assert bool(((c64 + 4).abs() < 1).any()) and bool(((c64.abs() - 35).abs() < 6).any()), case
            assert p.kind != "exact" or bool((c64 == 0).any()), case
        check("bound", prefix + "gelu_out", f"{case}-{p.kind}", "g", got_g, gref,
              U * gref.abs() + (1 + U) * gelu_err(c64))
        check("bound", prefix + "gelu_out", f"{case}-{p.kind}", "formula", gref + formula_need(got_g, gref), gref,
              gelu_err(c64))


# ---------------------------------------------------------------------------------------------------- the emulation
# fp32, in the kernels' order: two 32-wide MFMA steps per K-tile, K-tiles in sequence into one accumulator per slab /
# piece; the reducer's and the last arriver's sequential sums; the epilogue's separate multiply and add; bf16_round
# before the GELU formulas.  `defect` injects one of DEFECTS.
DEFECTS = ("drop_kt", "dup_kt", "drop_slab", "drop_piece", "dup_piece", "bf16_slabs", "bias_per_split", "alpha_on_c0",
           "chunk", "swap_tiles", "gelu_unrounded")


def emu_acc(a32, b32, kts):
    acc = torch.zeros(a32.shape[0], b32.shape[0])
    for kt in kts:
        for s in range(2):
            k = kt * BK + 32 * s
            acc = acc + a32[:, k:k + 32] @ b32[:, k:k + 32].t()
    return acc


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emu_gelu32(h):
    k0, k1 = torch.tensor(K0).float(), torch.tensor(K1).float()
    u = k0 * _fma32(k1 * h * h, h, h)
    return 0.5 * h * (2.0 - 2.0 * (1.0 / (1.0 + torch.exp(2.0 * u))))


def emu_gelu_grad32(h):
    k0, k1 = torch.tensor(K0).float(), torch.tensor(K1).float()
    e = torch.exp((2.0 * k0) * _fma32(k1 * h * h, h, h))
    t = 1.0 - 2.0 * (1.0 / (1.0 + e))
    q = 0.5 * h * (1.0 - t * t) * k0 * _fma32(3.0 * k1 * torch.ones_like(h), (h * h).clamp(max=3.0e38),
                                              torch.ones_like(h))
    return _fma32(torch.full_like(h, 0.5), 1.0 + t, q)


def emulate(p, path, alpha=1.0, bias=None, c0=None, gelu=False, h=None, defect=None, group=4):
    """(C bf16, gelu_out bf16 or None) of the path's dataflow in fp32 on the CPU."""
    M, N, K, nk = p.M, p.N, p.K, p.K // BK
    a32, b32 = p.a.float(), p.b.float()
    if defect == "chunk":                                          # one 16-byte chunk (8 k) of K-tile 1 from row + 1
        a32 = a32.clone()
        a32[5, BK + 8:BK + 16] = a32[6, BK + 8:BK + 16]
    nbias = 1
    if path == "exv":
        kps, lens = split_plan(M, N, K)
        slabs = []
        for s, ln in enumerate(lens):
            kts = list(range(s * kps, s * kps + ln))
            if defect == "drop_kt" and s == len(lens) - 1:
                kts = kts[1:]
            if defect == "dup_kt" and s == 0:
                kts = kts + kts[2:3]
            slabs.append(emu_acc(a32, b32, kts))
        if defect == "drop_slab":
            slabs = slabs[:-1]
        if defect == "bf16_slabs":
            slabs = [s.to(BF).float() for s in slabs]
        if defect == "bias_per_split":
            nbias = len(lens)
        acc = slabs[0]
        if len(lens) > 1:
            acc = torch.zeros(M, N)
            for s in slabs:
                acc = acc + s
    else:
        g, skt, ipb = sk_plan(M, N, K)
        ntm, ntn = M // TILE, N // TILE
        acc = torch.zeros(M, N)
        for t in range(ntm * ntn):
            tm, tn = tile_of(t, ntm, ntn, group)
            ar, br = a32[tm * TILE:(tm + 1) * TILE], b32[tn * TILE:(tn + 1) * TILE]
            pcs = sk_pieces(t, nk, ipb) if t < skt else [(0, nk)]
            parts = [emu_acc(ar, br, range(b, e)) for b, e in pcs]
            if t == 0 and defect == "drop_piece":
                parts = parts[:1] + parts[2:]
            if t == 0 and defect == "dup_piece":
                parts = parts[:2] + parts[1:]
            tot = parts[0]
            if len(pcs) > 1:
                tot = torch.zeros(TILE, TILE)
                for x in parts:
                    tot = tot + x
            acc[tm * TILE:(tm + 1) * TILE, tn * TILE:(tn + 1) * TILE] = tot
    al = torch.tensor(alpha).float()
    if c0 is not None:
        v = al * (acc + c0.float()) if defect == "alpha_on_c0" else al * acc + c0.float()
    else:
        v = acc * al
        if bias is not None:
            v = v + bias * nbias
    g_out = None
    if h is not None:
        v = v.to(BF).float() * emu_gelu_grad32(h.float())
    c = v.to(BF)
    if gelu:
        g_out = emu_gelu32(v if defect == "gelu_unrounded" else c.float()).to(BF)
    if defect == "swap_tiles":
        c = c.clone()
        c[:TILE, :TILE], c[:TILE, TILE:2 * TILE] = c[:TILE, TILE:2 * TILE].clone(), c[:TILE, :TILE].clone()
    return c, g_out


# ------------------------------------------------------------------------------------------------------- case tables
ONE_PASS = [(256, 256, 64), (256, 256, 128), (256, 256, 192), (256, 256, 320), (256, 512, 960)]   # 1 .. 5, 15 K-tiles
GROUP_SHAPE = (1280, 512, 320)                # 5 M-tiles x 2: a short last group, 10 workgroups over 8 XCDs
SPLIT_K = {(256, 256, 1088): [10, 7], (256, 256, 2112): [10, 10, 10, 3], (256, 256, 2624): [10, 10, 10, 10, 1],
           (256, 512, 8192): [8] * 16, (512, 768, 1024): [8, 8]}   # the last: 6 tiles, which the planner splits too
SK_FORCED = [(256, 256, 256), (256, 256, 384), (256, 256, 8192), (512, 768, 1408)]
SK_RULE = (768, 768, 2560)


def sk_big_shape(g):
    """8 M-tiles x enough N-tiles for two full data-parallel rounds and a partial wave of 8 tiles (G = 256: 520)."""
    ntn = next(n for n in range(1, 8 * g) if 8 * n > 2 * g and (8 * n) % g == 8 % g and (8 * n) // g == 2)
    return 2048, TILE * ntn, 512


class forced:
    """plx_gemm256_set_sk_force / set_group for a with-block, restored afterwards."""

    def __init__(self, force=None, group=None):
        self.force, self.group = force, group

    def __enter__(self):
        lib = _lib()
        self.pf = lib.plx_gemm256_set_sk_force(self.force) if self.force is not None else None
        self.pg = lib.plx_gemm256_set_group(self.group) if self.group is not None else None
        return self

    def __exit__(self, *exc):
        lib = _lib()
        if self.pf is not None:
            lib.plx_gemm256_set_sk_force(self.pf)
        if self.pg is not None:
            lib.plx_gemm256_set_group(self.pg)


# -------------------------------------------------------------------------------------------------------- CPU tests
CPU = torch.device("cpu")


def _emu_case(kind, path, shape, alpha=1.0, bias=False, acc=False, gelu=False, gelu_h=False, defect=None,
              scale=None):
    """(C, gelu_out, problem, bias, c0, h, chain) of one emulated case."""
    M, N, K = shape
    p = problem(CPU, kind, M, N, K, scale if scale is not None else (gelu_scale(kind, K) if gelu else 1.0))
    bv = p.extras("bias", "gelu" if gelu else None) if bias else None
    c0 = p.extras("c0") if acc else None
    h = p.extras("h") if gelu_h else None
    c, g = emulate(p, path, alpha, bv, c0, gelu, h, defect)
    return c, g, p, bv, c0, h, chain_of(path, M, N, K, 4, CPU)


def _emu_judge(kind, path, shape, fam, **kw):
    c, g, p, bv, c0, h, chain = _emu_case(kind, path, shape, **kw)
    judge(p, fam, "x".join(map(str, shape)), kw.get("alpha", 1.0), bv, c0, chain, c, g, h, prefix="emu-")


def test_emulation_is_inside_the_bound_and_exact_on_integers():
    """The fp32 emulation of every dataflow: bit-equal on exact data, ratio <= 1 on gauss and pos."""
    for kind in ("exact", "gauss", "pos"):
        for shape in [(256, 256, 64), (256, 256, 320)]:
            _emu_judge(kind, "exv", shape, "8-wave")
            _emu_judge(kind, "exv", shape, "8-wave", alpha=-2.0, bias=True)
            _emu_judge(kind, "exv", shape, "8-wave", alpha=0.5, acc=True)
        for shape in [(256, 256, 1088), (256, 256, 2624), (256, 512, 8192)]:
            _emu_judge(kind, "exv", shape, "split-K")
            _emu_judge(kind, "exv", shape, "split-K", alpha=0.5, bias=True)
            _emu_judge(kind, "exv", shape, "split-K", alpha=-2.0, acc=True)
        with forced(force=1):
            for shape in [(256, 256, 384), (256, 256, 8192), (512, 768, 1408)]:
                _emu_judge(kind, "sk", shape, "stream-K")
            _emu_judge(kind, "sk", (256, 256, 384), "stream-K", alpha=0.5, bias=True)
    for kind in KINDS:
        _emu_judge(kind, "exv", (256, 256, 320), "8-wave", bias=True, gelu=True)
        _emu_judge(kind, "exv", (256, 256, 1088), "split-K", bias=True, gelu=True)
        with forced(force=1):
            _emu_judge(kind, "sk", (256, 256, 384), "stream-K", gelu_h=True)
            _emu_judge(kind, "sk", (256, 256, 384), "stream-K", gelu=True)
    print("GEMM_EMU " + " ".join(f"{f[4:]}/{name}={v:.3f}" for (f, name), v in sorted(RATIOS.items())
                                 if f.startswith("emu-")))


def test_formula_bounds_hold_for_an_fp32_evaluation():
    """err_gelu / err_grad against a plain fp32 evaluation of the two formulas on every bf16 value in [-45, 45] and on
    the huge ones (the emulation caps h * h as the kernel does)."""
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(BF)
    h = bits[torch.isfinite(bits.float())].float()
    small = h[h.abs() <= 45.0]
    for f32, f64, err in ((emu_gelu32, gelu64, gelu_err), (emu_gelu_grad32, gelu_grad64, gelu_grad_err)):
        r = ratio(f32(small).double(), f64(small.double()), err(small.double()))
        assert float(r.max()) <= 1.0, (f32.__name__, float(r.max()), float(small[r.argmax()]))
    huge = h[h.abs() >= 2.0e19]
    want = (huge > 0).float()
    assert torch.equal(emu_gelu_grad32(huge), want) and torch.equal(gelu_grad64(huge.double()).float(), want)


# the defect, the path and shape it is injected into, and the epilogue it needs
DEFECT_CASES = {
    "drop_kt": ("exv", (256, 256, 1088), {}),
    "dup_kt": ("exv", (256, 256, 1088), {}),
    "drop_slab": ("exv", (256, 256, 1088), {}),
    "bf16_slabs": ("exv", (256, 512, 8192), {}),
    "bias_per_split": ("exv", (256, 256, 1088), {"bias": True}),
    "alpha_on_c0": ("exv", (256, 256, 1088), {"alpha": 0.5, "acc": True}),
    "drop_piece": ("sk", (256, 256, 8192), {}),
    "dup_piece": ("sk", (256, 256, 8192), {}),
    "chunk": ("exv", (256, 256, 960), {}),
    "swap_tiles": ("exv", (256, 512, 8192), {}),
    "gelu_unrounded": ("exv", (256, 256, 960), {"bias": True, "gelu": True}),
}


def _defect_verdicts(defect, kind):
    """(outside the new check, accepted by the old tolerance) of one injected defect on one kind of data."""
    path, shape, kw = DEFECT_CASES[defect]
    with forced(force=1):
        c, g, p, bv, c0, h, chain = _emu_case(kind, path, shape, defect=defect, **kw)
    alpha = kw.get("alpha", 1.0)
    ref, mag = reference(p, alpha, bv, c0)
    if defect == "gelu_unrounded":                                 # C itself is right; its GELU output is judged
        c64 = c.to(F64)
        gref = gelu64(c64)
        outside = float(ratio(g, gref, U * gref.abs() + (1 + U) * gelu_err(c64)).max()) > 1.0
        old = bool(torch.isclose(g.float(), gref.float(), rtol=1e-2, atol=1e-2).all())
        return outside, old
    if kind == "exact":
        outside = bool((c.to(F64) != rne(ref)).any())
    else:
        outside = float(ratio(c, ref, bound_c(ref, mag, chain, c0 is not None)).max()) > 1.0
    old = float((c.to(F64) - ref).abs().max()) <= 1.5e-2 * float(ref.abs().max()) + 1e-3
    return outside, old


@pytest.mark.parametrize("defect", DEFECTS)
def test_injected_defects_are_outside(defect):
    """Every defect is unequal on exact data and outside the bound on gauss and one-sign data (the GELU output, a
    bounded comparison on every kind, on exact and gauss: on one-sign data the activation is saturated, gelu(c) = c)."""
    kinds = ("gauss", "exact") if defect == "gelu_unrounded" else ("exact", "pos", "gauss")  # pos: gelu(c) = c
    for kind in kinds:
        outside, _ = _defect_verdicts(defect, kind)
        assert outside, (defect, kind)


# what tests/test_gpu_gemm.py's tolerance (max-norm for C, rtol = atol = 1e-2 for the GELU output) makes of each
# defect on randn data: True = accepted
OLD_ACCEPTS = {
    "drop_kt": False, "dup_kt": False, "drop_slab": False, "drop_piece": False, "dup_piece": False,
    "bf16_slabs": True, "bias_per_split": False, "alpha_on_c0": False, "chunk": False, "swap_tiles": False,
    "gelu_unrounded": True,
}


def test_old_tolerance_on_record():
    """The verdict of the old _check rule on every injected defect (gauss data, the shapes of DEFECT_CASES), next to
    the new check's: the record of what the max-norm rule lets through."""
    for defect in DEFECTS:
        outside, old = _defect_verdicts(defect, "gauss")
        print(f"GEMM_DEFECT {defect} new_check_rejects={outside} old_tolerance_accepts={old}")
        assert outside and old == OLD_ACCEPTS[defect], (defect, outside, old)


def test_case_tables_reach_their_plans():
    """Every listed case runs the plan it is listed for at 256 CUs (the planner's answer without a device)."""
    lib = _lib()
    if not torch.cuda.is_available():
        assert sk_plan(256, 256, 256)[0] == CUS
    for M, N, K in ONE_PASS + [GROUP_SHAPE]:
        assert lib.plx_gemm256_splits(M, N, K) == 1 and lib.plx_gemm256_kt_per_split(M, N, K) == K // BK
    ntm, ntn = GROUP_SHAPE[0] // TILE, GROUP_SHAPE[1] // TILE
    assert ntm % 4 and (ntm * ntn) % 8
    for group in (1, 4, 64):
        assert sorted(tile_of(i, ntm, ntn, group) for i in range(ntm * ntn)) == \
            [(m, n) for m in range(ntm) for n in range(ntn)]
    for (M, N, K), lens in SPLIT_K.items():
        assert split_plan(M, N, K)[1] == lens
    assert lib.plx_gemm256_kt_per_split(100, 256, 64) == 0
    with forced(force=1):
        g = sk_plan(256, 256, 256)[0]
        if g == CUS:
            assert sk_plan(256, 256, 256) == (g, 1, 4) and sk_pieces(0, 4, 4) == [(0, 4)]
            assert sk_plan(256, 256, 384) == (g, 1, 4) and sk_pieces(0, 6, 4) == [(0, 4), (4, 6)]
            assert sk_plan(256, 256, 8192) == (g, 1, 4) and len(sk_pieces(0, 128, 4)) == 32
            assert sk_plan(512, 768, 1408) == (g, 6, 4)
            assert sk_pieces(0, 22, 4)[-1] == (20, 22) and sk_pieces(1, 22, 4)[0] == (0, 2)   # one workgroup: 20 .. 24
            assert sk_big_shape(g) == (2048, 16640, 512)
            M, N, K = sk_big_shape(g)
            assert sk_plan(M, N, K) == (g, 8, 4) and (M // TILE) * (N // TILE) == 520
            assert all(len(sk_pieces(t, 8, 4)) == 2 for t in range(8))
    g, skt, ipb = sk_plan(*SK_RULE)                                # the cost rule itself
    assert skt > 0 and ((skt, ipb) == (9, 4) or g != CUS)


# ---------------------------------------------------------------------------------------------------- the GPU cases
GUARD = 0x7B7B


def _guarded(rows, ld, col0, n, dev):
    """A [rows][n] view at column col0 of a [rows + 2][ld] bf16 buffer filled with a guard pattern, and the buffer."""
    buf = torch.full((rows + 2, ld), GUARD, dtype=torch.int16, device=dev).view(BF)
    return buf[1:rows + 1, col0:col0 + n], buf


def _guards_intact(buf, rows, col0, n):
    raw = buf.view(torch.int16).clone()
    raw[1:rows + 1, col0:col0 + n] = GUARD
    return bool((raw == GUARD).all())


def _operand(x, kmajor, pad):
    """x [R][K] stored K-major ([R][K + pad]) or MN-major ([K][R + pad]); the padding is NaN.  (buffer, ld)"""
    r, k = x.shape
    buf = torch.full((r, k + pad) if kmajor else (k, r + pad), math.nan, dtype=BF, device=x.device)
    if kmajor:
        buf[:, :k] = x
    else:
        buf[:, :r] = x.t()
    return buf, buf.shape[1]


class Env:
    """The library, the CU count, and the test's own workspaces and tickets."""

    def __init__(self, dev):
        self.dev, self.lib = dev, _lib()
        self.G = sk_plan(256, 256, 256)[0]
        self.tickets = torch.zeros(self.G + 64, dtype=torch.int32, device=dev)
        self._ws = None

    def ws(self, floats):
        if self._ws is None or self._ws.numel() < floats:
            self._ws = None
            self._ws = torch.empty(max(floats, 1), dtype=torch.float32, device=self.dev)
        self._ws[:max(floats, 1)].fill_(math.nan)
        return self._ws

    def stream(self):
        return _native.current_stream()


@pytest.fixture(scope="module")
def env(cuda):
    return Env(cuda)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def launch(env, kind, shape, lay, path="exv", variant=8, alpha=1.0, bias=None, gelu=False, gelu_h=False, acc=False,
           pads=(0, 0, 0), scale=None, fam=None):
    """One call of plx_gemm256_exv / plx_gemm256_sk on guarded buffers; returns what judge_launch needs."""
    M, N, K = shape
    ak, bk = lay
    dev, lib = env.dev, env.lib
    p = problem(dev, kind, M, N, K, scale if scale is not None else (gelu_scale(kind, K) if gelu else 1.0))
    abuf, lda = _operand(p.a, ak, pads[0])
    bbuf, ldb = _operand(p.b, bk, pads[1])
    bv = p.extras("bias", "gelu" if gelu else None) if bias else None
    c0 = p.extras("c0") if acc else None
    h = p.extras("h") if gelu_h else None
    ldc, col0 = N + pads[2], 8 if pads[2] else 0
    out, obuf = _guarded(M, ldc, col0, N, dev)
    out.copy_(c0) if acc else out.fill_(math.nan)
    gout = gbuf = hv = None
    if gelu:
        gout, gbuf = _guarded(M, ldc, col0, N, dev)
        gout.fill_(math.nan)
    if gelu_h:
        hv, _ = _guarded(M, ldc, col0, N, dev)
        hv.copy_(h)
    group = lib.plx_gemm256_set_group(0)                           # out of range: reads the knob, changes nothing
    if path == "exv":
        ns = lib.plx_gemm256_splits(M, N, K)
        ws = env.ws(ns * M * N) if ns > 1 else None
        rc = lib.plx_gemm256_exv(abuf.data_ptr(), bbuf.data_ptr(), out.data_ptr(), _ptr(ws), M, N, K, lda, ldb, ldc,
                                 ak, bk, alpha, int(acc), _ptr(bv), _ptr(gout), variant, env.stream())
        fam = fam or ("split-K" if ns > 1 else "8-wave" if variant == 8 else "4-wave")
    else:
        floats = lib.plx_gemm256_sk_ws(M, N, K)
        ws = env.ws(floats) if floats else None
        rc = lib.plx_gemm256_sk(abuf.data_ptr(), bbuf.data_ptr(), out.data_ptr(), _ptr(ws), env.tickets.data_ptr(), M,
                                N, K, lda, ldb, ldc, ak, bk, alpha, _ptr(bv), _ptr(gout), _ptr(hv), env.stream())
        fam = fam or "stream-K"
    case = f"{M}x{N}x{K}-{'K' if ak else 'M'}{'K' if bk else 'N'}-v{variant if path == 'exv' else 9}"
    assert rc == 0, (case, rc)
    chain = chain_of(path, M, N, K, group, dev)
    return dict(p=p, fam=fam, case=case, alpha=alpha, bias=bv, c0=c0, chain=chain, out=out, obuf=obuf, gout=gout,
                gbuf=gbuf, h=h, geom=(M, col0, N), sk=path == "sk", keep=(abuf, bbuf, hv))


def judge_launch(env, L):
    M, col0, N = L["geom"]
    if L["sk"]:
        assert int(env.tickets.abs().sum()) == 0, f"{L['case']}: tickets left non-zero"
    assert _guards_intact(L["obuf"], M, col0, N), f"{L['case']}: C guard overwritten"
    if L["gbuf"] is not None:
        assert _guards_intact(L["gbuf"], M, col0, N), f"{L['case']}: gelu_out guard overwritten"
    judge(L["p"], L["fam"], L["case"], L["alpha"], L["bias"], L["c0"], L["chain"], L["out"], L["gout"], L["h"])


def run(env, *args, **kw):
    judge_launch(env, launch(env, *args, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ONE_PASS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", [8, 5])
def test_one_pass_tiles(env, variant, shape):
    """1, 2, 3, 5 and 16 K-tiles (the ring's fill and drain edges) on both kernels: every layout, exact and gauss; on
    two layouts also alpha + bias, accumulate, and the GELU output."""
    assert env.lib.plx_gemm256_splits(*shape) == 1
    torch.cuda.synchronize()
    for lay in LAYOUTS:
        for kind in KINDS:
            run(env, kind, shape, lay, variant=variant)
        if lay in ((1, 1), (0, 0)):
            run(env, "exact", shape, lay, variant=variant, alpha=-2.0, bias=True)
            run(env, "gauss", shape, lay, variant=variant, alpha=0.5, bias=True)
            run(env, "exact", shape, lay, variant=variant, alpha=0.5, acc=True)
            run(env, "pos", shape, lay, variant=variant, alpha=-2.0, acc=True)
            for kind in KINDS:
                run(env, kind, shape, lay, variant=variant, bias=True, gelu=True)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [8, 5])
def test_tile_order_knob(env, variant):
    """5 M-tiles x 2 N-tiles: 10 workgroups (the XCD remap's remainder) and a short last group, at group 1, 4, 64."""
    for group in (1, 4, 64):
        with forced(group=group):
            assert env.lib.plx_gemm256_set_group(0) == group
            for lay in LAYOUTS:
                for kind in KINDS:
                    run(env, kind, GROUP_SHAPE, lay, variant=variant)
    assert env.lib.plx_gemm256_set_group(0) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SPLIT_K), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", [8, 5])
def test_split_k(env, variant, shape):
    """Split-K slabs and the reducer: last splits of 7, 3 and 1 K-tiles and 16 even ones; plain (every layout), alpha
    + bias, the GELU output, accumulate (with which a bias is rejected)."""
    assert split_plan(*shape)[1] == SPLIT_K[shape]
    for lay in LAYOUTS:
        for kind in KINDS:
            run(env, kind, shape, lay, variant=variant)
    for lay in ((0, 0), (1, 1)):
        run(env, "pos", shape, lay, variant=variant)
        run(env, "exact", shape, lay, variant=variant, alpha=-2.0, bias=True)
        run(env, "gauss", shape, lay, variant=variant, alpha=0.5, bias=True)
        for kind in KINDS:
            run(env, kind, shape, lay, variant=variant, bias=True, gelu=True)
            run(env, kind, shape, lay, variant=variant, alpha=0.5, acc=True)
    M, N, K = shape
    p = problem(env.dev, "exact", M, N, K)
    out = torch.full((M, N), math.nan, dtype=BF, device=env.dev)
    bias = torch.zeros(N, device=env.dev)
    ws = env.ws(len(SPLIT_K[shape]) * M * N)
    rc = env.lib.plx_gemm256_exv(p.a.data_ptr(), p.b.data_ptr(), out.data_ptr(), ws.data_ptr(), M, N, K, K, K, N, 1, 1,
                                 1.0, 1, bias.data_ptr(), None, variant, env.stream())
    assert rc == -1 and bool(torch.isnan(out).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SK_FORCED, ids=lambda s: "x".join(map(str, s)))
def test_stream_k_forced(env, shape):
    """The persistent kernel with every partial wave split: one piece, 4 + 2, one tile in 32 pieces, pieces across
    tile boundaries; bias, alpha, both GELU epilogues; the tickets zero after every launch."""
    M, N, K = shape
    with forced(force=1):
        g, skt, ipb = sk_plan(M, N, K)
        assert skt == ((M // TILE) * (N // TILE)) % g and skt > 0 and ipb % 2 == 0
        np_ = [len(sk_pieces(t, K // BK, ipb)) for t in range(skt)]
        if g == CUS:
            assert np_ == {256: [1], 384: [2], 8192: [32], 1408: [6, 6, 6, 6, 6, 6]}[K]
        lays = LAYOUTS if shape in (SK_FORCED[1], SK_FORCED[3]) else [(1, 1), (1, 0)]
        for lay in lays:
            for kind in KINDS:
                run(env, kind, shape, lay, path="sk")
        run(env, "pos", shape, (1, 1), path="sk")
        run(env, "exact", shape, (1, 1), path="sk", alpha=-2.0, bias=True)
        run(env, "gauss", shape, (1, 0), path="sk", alpha=0.5, bias=True)
        for kind in KINDS:
            run(env, kind, shape, (1, 1), path="sk", bias=True, gelu=True)
            run(env, kind, shape, (0, 0), path="sk", gelu=True)
            run(env, kind, shape, (1, 0), path="sk", gelu_h=True)
            run(env, kind, shape, (0, 1), path="sk", gelu_h=True, alpha=0.5)


@pytest.mark.gpu
def test_stream_k_split_pieces_beside_data_parallel_chains(env):
    """520 tiles on 256 CUs (computed from the CU count): 8 tiles split in two, then two chained data-parallel tiles
    per workgroup; the first 16 workgroups run a split piece and then their tiles.  fp64 reference on the GPU."""
    M, N, K = sk_big_shape(env.G)
    with forced(force=1):
        g, skt, ipb = sk_plan(M, N, K)
        T, nk = (M // TILE) * (N // TILE), K // BK
        assert skt == 8 % g and (T - skt) // g == 2 and all(len(sk_pieces(t, nk, ipb)) == 2 for t in range(skt))
        run(env, "exact", (M, N, K), (1, 1), path="sk", alpha=0.5, bias=True)
        run(env, "gauss", (M, N, K), (1, 0), path="sk")
    _PROBLEMS.clear()


@pytest.mark.gpu
def test_stream_k_cost_rule_and_tile_order(env):
    """768x768x2560 is split by the planner's own rule (9 tiles of 40 K-tiles); 1280x512x384 forced, at group 1, 4
    and 64 (5 M-tiles: a short last group inside the persistent kernel's tile walk)."""
    assert env.lib.plx_gemm256_set_sk_force(0) == 0
    g, skt, ipb = sk_plan(*SK_RULE)
    assert skt == 9 % g and skt > 0 and SK_RULE[2] // BK - ipb >= 16
    for lay in LAYOUTS:
        for kind in KINDS:
            run(env, kind, SK_RULE, lay, path="sk")
    run(env, "gauss", SK_RULE, (1, 1), path="sk", bias=True, gelu=True)
    for group in (1, 4, 64):
        with forced(force=1, group=group):
            for kind in KINDS:
                run(env, kind, (1280, 512, 384), (1, 1), path="sk")
                run(env, kind, (1280, 512, 384), (0, 0), path="sk", alpha=-2.0, bias=True)
    assert env.lib.plx_gemm256_set_group(0) == 4



@pytest.mark.gpu
def test_stream_k_back_to_back_on_one_ticket_array(env):
    """Three shapes launched back to back on the same tickets and workspace, judged afterwards: each launch finds
    the tickets its predecessor reset."""
    with forced(force=1):
        shapes = [(256, 256, 384), (512, 768, 1408), (256, 256, 8192), (512, 768, 1408)]
        ws = env.ws(env.lib.plx_gemm256_sk_ws(512, 768, 1408))
        done = []
        for i, (M, N, K) in enumerate(shapes):
            p = problem(env.dev, "exact", M, N, K)
            out = torch.full((M, N), math.nan, dtype=BF, device=env.dev)
            rc = env.lib.plx_gemm256_sk(p.a.data_ptr(), p.b.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                        env.tickets.data_ptr(), M, N, K, K, K, N, 1, 1, 1.0, None, None, None,
                                        env.stream())
            assert rc == 0
            done.append((p, out))
        torch.cuda.synchronize()
        assert int(env.tickets.abs().sum()) == 0
        for p, out in done:
            ref, _ = reference(p, 1.0, None, None)
            check("exact", "stream-K", f"back-to-back-{p.M}x{p.N}x{p.K}", "c", out, ref, None, p)


@pytest.mark.gpu
def test_padded_leading_dimensions_and_guards(env):
    """lda, ldb and ldc larger than the row (NaN in the operands' padding, a guard pattern around C, gelu_out and
    gelu_h laid out like C) on every path and layout."""
    pads = (8, 72, 64)
    for lay in LAYOUTS:
        for kind in KINDS:
            for variant in (8, 5):
                run(env, kind, (256, 512, 320), lay, variant=variant, pads=pads)
                run(env, kind, (256, 256, 1088), lay, variant=variant, pads=pads, bias=True, gelu=True)
            run(env, kind, (256, 256, 1088), lay, pads=pads, alpha=0.5, acc=True)
            with forced(force=1):
                run(env, kind, (512, 768, 1408), lay, path="sk", pads=pads, bias=True, gelu=True)
                run(env, kind, (512, 768, 1408), lay, path="sk", pads=pads, gelu_h=True)


@pytest.mark.gpu
def test_ops_wrapper(env, monkeypatch):
    """ops/gemm.py on exact data: the forward with bias and GELU output (stream-K schedule), the weight gradient
    accumulated through split-K into a column block of a wider matrix, the fused GELU backward."""
    from polyaxon_amd.ops import gemm

    dev = env.dev
    monkeypatch.setenv("PLX_LM_GEMM", "1")
    monkeypatch.delenv("PLX_GEMM_WAVES", raising=False)
    p = problem(dev, "exact", 512, 768, 1024, gelu_scale("exact", 1024))
    bias = p.extras("bias", "gelu")
    hq = torch.full((512, 768), math.nan, dtype=BF, device=dev)
    gq = torch.full_like(hq, math.nan)
    gemm.gemm(p.a, p.b, 512, 768, 1024, True, True, out=hq, bias=bias, gelu_out=gq)
    judge(p, "stream-K", "ops-fwd-512x768x1024", 1.0, bias, None, chain_of("sk", 512, 768, 1024, 4, dev), hq, gq)
    p = problem(dev, "exact", 256, 512, 8192)
    c0 = p.extras("c0")
    wide, buf = _guarded(256, 512 + 64, 8, 512, dev)
    wide.copy_(c0)
    gemm.gemm(p.a.t().contiguous(), p.b.t().contiguous(), 256, 512, 8192, False, False, out=wide, accumulate=True,
              alpha=0.5)
    assert _guards_intact(buf, 256, 8, 512)
    judge(p, "split-K", "ops-wgrad-256x512x8192", 0.5, None, c0, chain_of("exv", 256, 512, 8192, 4, dev), wide)
    p = problem(dev, "exact", 512, 768, 256)
    h = p.extras("h")
    monkeypatch.setattr(gemm, "FORCE_SCHEDULE", gemm.SK)
    dh = gemm.gemm(p.a, p.b.t().contiguous(), 512, 768, 256, True, False, gelu_h=h)
    judge(p, "stream-K", "ops-gelu-bwd-512x768x256", 1.0, None, None, chain_of("sk", 512, 768, 256, 4, dev), dh,
          None, h)


@pytest.mark.gpu
def test_gelu_grad_at_huge_h(env):
    """|h| >= 2^64: h * h overflows and the derivative's second term was 0 * inf.  The true derivative is 1 (h > 0)
    or 0 (h < 0) -- and 0.5 at h = 0 -- exactly, in the GEMM epilogue and in the separate pass (plx_gelu_bwd_colsum),
    which must also agree with each other."""
    from polyaxon_amd.ops import lm

    dev = env.dev
    M, N, K = 256, 256, 256
    p = problem(dev, "exact", M, N, K)
    vals = torch.tensor([0.0, 2.5e19, -2.5e19, 3.0e38, -3.0e38, 1.9e19, -1.9e19, 1.0e25], device=dev)
    h = vals[torch.arange(M * N, device=dev) % 8].view(M, N).to(BF)
    assert float(h.float().abs().max()) > 2.0e19 and bool((h == 0).any())
    out = torch.full((M, N), math.nan, dtype=BF, device=dev)
    rc = env.lib.plx_gemm256_sk(p.a.data_ptr(), p.b.data_ptr(), out.data_ptr(), None, env.tickets.data_ptr(), M, N, K,
                                K, K, N, 1, 1, 1.0, None, None, h.data_ptr(), env.stream())
    assert rc == 0
    d = rne(reference(p, 1.0, None, None)[0])
    want = rne(d * torch.where(h == 0, 0.5, (h > 0).double()))
    bad = out.to(F64) != want
    assert not bool(bad.any()), \
        f"fused epilogue: {int(bad.sum())} wrong, {int(torch.isnan(out).sum())} NaN, {where(bad)}"
    dh2, _ = lm.bias_grad(d.to(BF), torch.zeros(N, device=dev, requires_grad=True), gelu_h=h)
    bad = dh2.to(F64) != want
    assert not bool(bad.any()), \
        f"separate pass: {int(bad.sum())} wrong, {int(torch.isnan(dh2).sum())} NaN, {where(bad)}"


@pytest.mark.gpu
def test_argument_checks_return_without_a_launch(env):
    """The documented rejections of both entry points: each returns its code and leaves the output untouched."""
    dev, lib = env.dev, env.lib
    M, N, K = 256, 256, 2112                                        # 4 splits; an even K-tile count is K = 2048
    p = problem(dev, "exact", M, N, K)
    a = torch.zeros(M * K + 8, dtype=BF, device=dev)
    a[:M * K] = p.a.reshape(-1)
    out, buf = _guarded(M, N + 64, 8, N, dev)
    out.fill_(math.nan)
    g2 = torch.full((M, N + 64), math.nan, dtype=BF, device=dev)
    bias = torch.zeros(N + 4, device=dev)
    ws = env.ws(4 * M * N)
    A, B, C, W, T = a.data_ptr(), p.b.data_ptr(), out.data_ptr(), ws.data_ptr(), env.tickets.data_ptr()
    ldc, st = N + 64, env.stream()

    def exv(A=A, B=B, C=C, W=W, K=K, lda=K, ldb=K, ldc=ldc, acc=0, bias=None, gelu=None):
        return lib.plx_gemm256_exv(A, B, C, W, M, N, K, lda, ldb, ldc, 1, 1, 1.0, acc, bias, gelu, 8, st)

    def sk(A=A, B=B, C=C, W=W, T=T, K=2048, lda=K, ldb=K, ldc=ldc, bias=None, gelu=None, h=None):
        return lib.plx_gemm256_sk(A, B, C, W, T, M, N, K, lda, ldb, ldc, 1, 1, 1.0, bias, gelu, h, st)

    assert exv(A=A + 2) == -1 and exv(B=B + 2) == -1 and exv(C=C + 2) == -1
    assert exv(lda=K + 4) == -1 and exv(ldb=K + 4) == -1 and exv(ldc=ldc + 4) == -1
    assert exv(bias=bias.data_ptr() + 4) == -1 and exv(gelu=g2.data_ptr() + 2) == -1
    assert exv(acc=1, bias=bias.data_ptr()) == -1 and exv(acc=1, gelu=g2.data_ptr()) == -1
    assert exv(K=K + 32) == -1 and exv(W=None) == -5
    assert lib.plx_gemm256_exv(A, B, C, W, M + 128, N, K, K, K, ldc, 1, 1, 1.0, 0, None, None, 8, st) == -1
    with forced(force=1):
        assert sk(A=A + 2) == -1 and sk(B=B + 2) == -1 and sk(C=C + 2) == -1 and sk(lda=K + 4) == -1
        assert sk(K=320) == -1 and sk(K=128) == -1 and sk(K=192) == -1            # odd, short, odd and short
        assert sk(bias=bias.data_ptr() + 4) == -1 and sk(gelu=g2.data_ptr() + 2) == -1
        assert sk(h=g2.data_ptr(), bias=bias.data_ptr()) == -1 and sk(h=g2.data_ptr(), gelu=g2.data_ptr()) == -1
        assert sk(h=g2.data_ptr() + 2) == -1
        assert sk(W=None) == -5 and sk(T=None) == -5
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and _guards_intact(buf, M, 8, N) and bool(torch.isnan(g2).all())
    assert int(env.tickets.abs().sum()) == 0
