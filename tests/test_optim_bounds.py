"""The fused SGD / AdamW kernels (csrc/train_kernels.hip) against float64 with a-priori, per-element bounds.

tests/test_gpu_kernels.py and tests/test_gpu_grad_clip.py compare the parameter with torch.optim in fp32 under
rtol = 1e-5, atol = 1e-6 after 1-3 steps from m = v = 0 with randn gradients: with an update of about 1e-3 that accepts
a relative error of 1e-3 in the update, m and v are never looked at, the step counter never passes 2 and the
grid-stride loop never takes a second trip (test_old_tolerance_misses_the_recorded_defects keeps on record what that
lets through).  Here the reference is float64 from the very bits the kernel receives -- fp32 p / m / v, the fp32 hp
vector, the int step, the fp32 or bf16 gradient, the clip state -- every output (p, m, v, plp, and the gradient, which
must be all zero bits) is held to its own bound, the statistic is max |got - ref| / bound and the assertion is <= 1.0.
Nothing in a bound is fitted to what the kernels return.

Notation.  E = 2^-24: fp32's unit roundoff.  U = 2^-8: bf16's (plp only, and plp is asserted bit for bit).  gamma(k) =
k E / (1 - k E) bounds |prod_{i<=k} (1 + d_i)^(+-1) - 1| for |d_i| <= E; a sum of products each of which went through at
most k roundings is wrong by at most gamma(k) times the sum of the absolute values of its terms.  TINY = 2^-126 is
added per operation whose result can fall below the normal range (gradual underflow and flush-to-zero alike): g * g
and (1 - b) g for the smallest gradients, b^t near its underflow.

Facts used, from the ROCm headers and the build flags.  __powf is __ocml_pow_f32 and rsqrtf is __ocml_rsqrt_f32
(__clang_hip_math.h).  The ROCm tree here carries no device-libs / OCML accuracy document (only ocml.bc), so their
limits are the OpenCL full-profile ones these functions are specified to: pow 16 ulp, rsqrt 2 ulp, one ulp being at
most 2 E relative (K_POW, K_RSQRT; not lowered to what the GPU delivers).  sqrtf and / are correctly rounded because
ops/_native.py builds without fast-math.  (float)(step + 1) is exact below 2^24.  Counts are of the uncontracted form:
sgd_flat and adamw_flat may be contracted by the compiler, which only removes roundings; the mixed kernels run
adamw_elem under fp contract(off) with explicit fmaf, and the count is exactly what adamw_elem does (x = 0 below; the
flat kernel's two extra product roundings are x = 1).  The clip multiply g' = fl(g scale) is one rounding of its own
(scale_grad), c = 1 with clipping and 0 without; the reference takes g scale in float64.

AdamW scalars, common to all elements (the "scalar part" of the bound of p).  t = step + 1, pw = b^t, bc = 1 - pw.
    |pw^ - pw| <= d_pw = 2 K_POW E pw + TINY,  bc^ = fl(1 - pw^):  |bc^ - bc| <= d_pw + E (bc + d_pw)
The cancellation in 1 - b^t: an error of K_POW ulp in b^t becomes 2 K_POW E b^t / (1 - b^t) relative in bc -- e_bc.
At t = 1, b2 = 0.999 that is 32 E 999 = 1.9e-3; at t = 10 it is 1.9e-4; it vanishes with b^t.  b1^t = 0.9^t rounds
to zero in fp32 (is below 2^-150) from t = 987 on and is below the normal range from t = 829; 0.95^t from 2028 (1703);
0.999^t from 103922 (87294), b being the fp32 value.  From the smaller t on b^t is below E / 2 by far, bc is exactly
1.0f whatever pow returns for it, and the float64 bc is 1.0 too: at t = 10^3 bc1 is 1 (and bc2 with b2 = 0.95), at
t = 10^5 and 10^7 all of them are, and the scalar part is E for step_size and 2 K_RSQRT E for inv_sqrt_bc2.
    step_size = fl(lr / bc1^):      e_ss = (1 + E) / (1 - e_bc1) - 1
    inv_sqrt_bc2 = rsqrt(bc2^):     e_is = (1 + 2 K_RSQRT E) / sqrt(1 - e_bc2) - 1
    decay D = 1 - lr wd:            d_D = gamma(2) (|D| + lr wd)          (0 off the decay range, where D = 1)

m and v (adamw_elem: m = fma(b1, m, fl(fl(1 - b1) g)), v = fma(b2, v, fl(fl(fl(1 - b2) g) g)); adamw_flat the same
products and one add).  The term b m sees at most 2 roundings, (1 - b1) g three (the fp32 rounding of 1.f - b1, the
product, the add) and (1 - b2) g g four; each rounding of g' counts once per factor g:
    b_m = gamma(3 + c) (|b1 m| + |(1 - b1) g|) + 3 TINY
    b_v = gamma(4 + 2 c) (b2 v + (1 - b2) g^2) + (3 + 2 |g|) TINY

p = fma(p, D, -fl(fl(step_size m) / denom)), denom = fma(sqrtf(v), inv_sqrt_bc2, eps).  The elementwise part carries
b_m and b_v through m / (sqrt(v) s + eps), the divide and the final multiply-add; e_ss, e_is, d_D are the scalar part.
    sqrt(v^):  d_sq = min(b_v / sqrt(v), sqrt(b_v)),  d_s = d_sq + E (sqrt(v) + d_sq)          (correctly rounded)
    A = sqrt(v) s:  d_A = d_s s (1 + e_is) + A e_is  [+ E (A + d_A) if x]
    denom = A + eps:  d_den = d_A + E (denom + d_A)                                   (eps is the fp32 input: exact)
    num = step_size m:  d_num = ss (1 + e_ss) b_m + ss |m| e_ss, then + E (|num| + d_num) + TINY
    q = num / denom:  d_q0 = (d_num + |q| d_den) / (denom - d_den),  d_q = d_q0 + E (|q| + d_q0) + TINY
    b_p = |p| d_D + d_q + E (|q| + d_q) + (1 + x) E (1 + E) (|p D| + |p| d_D) + TINY
With |p| ~ 0.02 (GPT-2's initialisation) and an update of 1e-3 the bound of p is about E |p| + 5 E |q| ~ 2e-9 at large
t: a relative error of 1e-6 in the update is outside it.  At t = 1 with b2 = 0.999 the scalar part honestly allows
1e-3 of the update; the cases at t = 10^3 ... 10^7 are the ones that hold the corrections to a few E.

plp is the round-to-nearest-even of the fp32 p the kernel wrote: asserted with torch.equal on the kernel's own p (the
float64 p is held to b_p separately), and plx_cast_lp of that p must reproduce it.

SGD (sgd_flat_kernel): gg = g' + fl(w p) on [0, n_decay), w = 0 past it; first step: m = gg, else m = fl(mom m) +
fl(fl(1 - damp) gg); d = gg + fl(mom m) with Nesterov, else m; p = p - fl(lr d).  A short chain of products and adds;
with G = |g scale| + |w p|, M = G (first step) or |mom m| + |1 - damp| G, Dn = G + |mom| M (Nesterov) or M:
    b_m = gamma(k_m) M + 3 TINY,  k_m = 2 + c (first step) or 5 + c
    b_p = gamma(k_d + 2) (|p| + |lr| Dn) + 4 TINY,  k_d = k_m + 2 (Nesterov) or k_m
Exact cases (bound 0): with lr, momentum, dampening, wd (and the clip scale) powers of two and p / g / m small
integers no operation rounds and p, m must equal the float64 ones (SGD_HPS "pow2").  AdamW: b1 = 0 gives m == g bit
for bit; lr = 0 leaves p bit-unchanged (with any wd: 1 - 0 wd is 1); g = 0 with m = v = 0 gives fl(p decay); the
narrow, wide non-temporal and wide plain mixed kernels agree bit for bit, on 16-byte and on 8-byte aligned pointers; a
clip scale of 1.0 is bit for bit the entry point without clipping; skip = 1 leaves p / m / v / plp bit-unchanged and
zeroes g.

Layout: cases and data, oracle and bounds, the fp32 emulation (CPU tests: inside every bound on every case; each
injected defect of DEFECTS outside on its named case; what the old tolerance accepts), the GPU cases (every buffer
between guard words, intact after each launch).

Largest measured ratio per kernel and output on an MI355X (OPTIM_RATIO lines of the GPU cases; the fp32 emulation's
over the same cases in brackets):

    kernel        output   ratio
    sgd_flat      p        0.408 (0.605)   the case above the fixed 2048-block grid among them
    sgd_flat      m        0.618 (0.864)
    adamw_flat    p        0.479 (0.565)
    adamw_flat    m        0.574 (0.630)
    adamw_flat    v        0.615 (0.615)
    adamw_mixed   p        0.638 (0.711)
    adamw_mixed   m        0.575 (0.575)
    adamw_mixed   v        0.605 (0.605)
    adamw_mixed   plp      bit-equal to bf16_rne(p) in every case, all three kernels
    cast_lp       plp      bit-equal to bf16_rne(p), above the grid cap too

m and v sit at a little over half their bounds -- gamma(3) and gamma(4) are worst case in every rounding, a value just
above a power of two uses all of one E -- and p below its own, whose scalar part (pow at 16 ulp, rsqrt at 2) the
emulation pushes to the limit and the GPU does not.  Every kernel met every bound and every exact case as first
written, the second and later grid-stride trips, the 8-byte aligned fallback and the step counter at 10^7 included; no
guard word was touched.  What reading launch_* found: the entry points launched on a null hp or step (read by every
lane whatever n) and on null buffers with n > 0, which the kernels would have dereferenced, and on a negative n,
which ran an empty loop; all three now return 1 (test_refused_arguments_launch_nothing).  What the old tolerance accepted of the injected defects is in
test_old_tolerance_misses_the_recorded_defects.
"""
import functools
import math
import zlib
from collections import namedtuple

import pytest
import torch

E = 2.0 ** -24           # fp32 unit roundoff
U = 2.0 ** -8            # bf16 round-to-nearest unit roundoff (plp: asserted bit for bit)
TINY = 2.0 ** -126       # an fp32 result below the normal range
K_POW, K_RSQRT = 16, 2   # OpenCL full-profile ulp limits of pow and rsqrt
GUARD16, GUARD32 = 0x7B7B, 0x7B7B7B7B
PAD = 256
_F32, _BF, _F64 = torch.float32, torch.bfloat16, torch.float64
SGD_CAP_ELEMS = 2048 * 256 * 4          # one trip of sgd_flat / cast_lp at their fixed cap of 2048 blocks


def _gamma(k):
    return k * E / (1 - k * E)


def _ratio(got, ref, bound) -> float:
    """max |got - ref| / bound.  A bound of exactly 0 means the element must be exact; NaN must sit exactly where the
    reference has it."""
    got = got.to(ref.device).double().reshape(ref.shape)
    nan = ref.isnan()
    if not torch.equal(got.isnan(), nan):
        return math.inf
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(nan, torch.zeros_like(r), r).nan_to_num(nan=math.inf)
    return float(r.max()) if r.numel() else 0.0


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == _BF else torch.int32)


def _same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits."""
    return (t.contiguous().view(torch.int32) & -65536).view(_F32).to(_BF)


# ----------------------------------------------------------------------------------------------------------- cases
# kernel: sgd | flat | mixed.  hp: a name in SGD_HPS / ADAM_HPS.  step: the device counter (sgd: 0 is the first step).
# g: the gradient kind (_grad).  decay: n_decay (sgd, flat) or decay_on (mixed).  clip: None (the entry point without
# clipping), a scale, or "skip".  cap: plx_set_adamw_grid_cap for the launch (None: the default 2048).
Case = namedtuple("Case", "kernel n hp step g decay clip cap")

#            lr     b1   b2     eps   wd
ADAM_HPS = {
    "gpt2": (6e-4, 0.9, 0.95, 1e-8, 0.1),
    "torch": (1e-3, 0.9, 0.999, 1e-8, 0.01),
    "b1zero": (1e-3, 0.0, 0.999, 1e-8, 0.01),
    "eps3": (1e-3, 0.9, 0.999, 1e-3, 0.01),       # with |g| ~ 1e-4: eps is ten times sqrt(v)
    "eps8": (1e-3, 0.9, 0.999, 1e-8, 0.01),       # with |g| in [1e-9, 1e-7]: eps = 1e-8 among the sqrt(v)
    "lr0": (0.0, 0.9, 0.999, 1e-8, 0.1),
    "wd0": (1e-3, 0.9, 0.999, 1e-8, 0.0),
    "lr0wd0": (0.0, 0.9, 0.999, 1e-8, 0.0),
}
#           lr    mom  wd    nesterov damp
SGD_HPS = {
    "plain": (0.1, 0.9, 1e-3, 0.0, 0.1),
    "nest": (0.1, 0.9, 1e-3, 1.0, 0.1),
    "pow2": (0.125, 0.5, 0.25, 1.0, 0.25),        # with integer p / g / m: exact
    "lr0": (0.0, 0.9, 1e-3, 1.0, 0.0),
    "wd0": (0.1, 0.9, 0.0, 0.0, 0.0),
    "mom0": (0.1, 0.0, 1e-3, 1.0, 0.5),
}
STEPS = (0, 1, 9, 999, 99_999, 9_999_999)
SIZES = (4, 8, 12, 4100, 4104)
N_BIG = SGD_CAP_ELEMS + 1028                      # sgd_flat / cast_lp: one full trip and a ragged one
N_CAP4, N_CAP8 = 3 * 2048 + 4, 3 * 4096 + 8       # cap 2: three full trips and a ragged one, 4-wide / 8-wide


def _n_decays(n):
    return sorted({0, 4, min(1028, n), n - 4, n})


def _make_cases():
    c = []
    for k in ("flat", "mixed"):
        full = (lambda n: n) if k == "flat" else (lambda n: 1)
        c += [Case(k, n, "gpt2", 1, "randn", full(n), None, None) for n in SIZES]
        c += [Case(k, 4100, hp, s, "log", full(4100), None, None) for hp in ("gpt2", "torch") for s in STEPS]
        c += [Case(k, 4104, "torch", 9, "randn", d, None, None) for d in (_n_decays(4104) if k == "flat" else (0, 1))]
        for s in (0, 9):
            c += [Case(k, 4104, hp, s, g, full(4104), None, None)
                  for hp, g in (("b1zero", "randn"), ("eps3", "small4"), ("eps8", "tiny"), ("lr0", "randn"),
                                ("wd0", "randn"), ("lr0wd0", "log"))]
        c += [Case(k, 4104, "gpt2", 9, "randn", full(4104) if k == "mixed" else 1028, clip, None)
              for clip in (1.0, 0.37, "skip")]
        c += [Case(k, 4100, "torch", 999, "log", full(4100) if k == "mixed" else 4, 0.37, None)]
        c += [Case(k, N_CAP4, "gpt2", 9, "randn", full(N_CAP4) if k == "mixed" else N_CAP4 - 4, None, 2),
              Case(k, N_CAP8, "torch", 999, "log", full(N_CAP8) if k == "mixed" else 1028, 0.37, 2)]
    c += [Case("mixed", 768, hp, s, "sweep", 1, None, None) for hp, s in (("gpt2", 0), ("torch", 9), ("eps8", 999))]
    c += [Case("sgd", n, hp, s, "randn", n, None, None) for n in SIZES for hp, s in (("plain", 0), ("nest", 5))]
    c += [Case("sgd", 4104, "nest", 5, "randn", d, None, None) for d in _n_decays(4104)]
    c += [Case("sgd", 4104, hp, s, "log", 1028, None, None) for hp in ("plain", "nest") for s in (0, 5)]
    c += [Case("sgd", 4104, hp, s, "randn", 1028, None, None) for hp in ("lr0", "wd0", "mom0") for s in (0, 5)]
    c += [Case("sgd", 4104, "nest", s, "randn", 1028, clip, None) for s in (0, 5) for clip in (1.0, 0.37, "skip")]
    c += [Case("sgd", 4104, "pow2", s, "ints", 1028, clip, None) for s in (0, 5) for clip in (None, 0.5)]
    c += [Case("sgd", N_BIG, "nest", 3, "randn", N_BIG - 4, 0.37, None)]
    return c


CASES = list(dict.fromkeys(_make_cases()))       # the size and the n_decay lists meet in one case
SMALL = [c for c in CASES if c.n < 100_000]
assert len(set(CASES)) == len(CASES)


def _cid(c: Case) -> str:
    return f"{c.kernel}-n{c.n}-{c.hp}-s{c.step}-{c.g}-d{c.decay}-c{c.clip}-cap{c.cap}"


def _bf16_sweep():
    """Every bf16 bit pattern of [0, 2^-124) -- zero and all subnormals among them -- of [1, 4) and of (-2, -1]."""
    bits = torch.cat([torch.arange(0x0000, 0x0180), torch.arange(0x3F80, 0x4080), torch.arange(0xBF80, 0xC000)])
    return (bits - ((bits >= 0x8000) * 0x10000)).to(torch.int16).view(_BF)


def _grad(gen, n, kind):
    """fp32 gradient and its typical magnitude.  Every random kind has exact zeros mixed in."""
    u = torch.rand(n, generator=gen, dtype=_F64)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    if kind == "sweep":
        g = _bf16_sweep().float()
        assert g.numel() == n
        return g, 1.0
    if kind == "ints":
        return torch.randint(-8, 9, (n,), generator=gen).float(), 4.0
    if kind == "log":                                           # log-uniform over [2^-60, 2^10]
        g, sigma = sign * torch.exp2(-60.0 + 70.0 * u), 1.0
    elif kind == "tiny":                                        # log-uniform over [1e-9, 1e-7]
        g, sigma = sign * 10.0 ** (-9.0 + 2.0 * u), 1e-8
    else:
        sigma = 1e-4 if kind == "small4" else 1.0
        g = torch.randn(n, generator=gen, dtype=_F64) * sigma
    zero = torch.rand(n, generator=gen) < 0.125
    zero[::5] |= n > 12
    return torch.where(zero, 0.0, g).float(), sigma


@functools.lru_cache(maxsize=None)
def _small_data(case: Case):
    return _data(case)


def _data(case: Case):
    """The exact inputs of a launch, on the host: p, g, m, v (fp32; g bf16 for mixed), hp (8 fp32), step, state."""
    gen = _gen("optim", case)
    n = case.n
    g, sigma = _grad(gen, n, case.g)
    d = dict(step=case.step, decay=case.decay)
    if case.g == "ints":
        d["p"] = torch.randint(-8, 9, (n,), generator=gen).float()
        d["m"] = torch.randint(-8, 9, (n,), generator=gen).float()
    else:
        d["p"] = torch.randn(n, generator=gen) * 0.02           # GPT-2's initialisation
        d["m"] = torch.randn(n, generator=gen) * (0.3 * sigma)
    if case.kernel == "sgd":
        hp = SGD_HPS[case.hp]
    else:
        hp = ADAM_HPS[case.hp]
        if case.step == 0:                                      # m and v consistent with the step: zero before it
            d["m"] = torch.zeros(n)
            d["v"] = torch.zeros(n)
        else:
            bc2 = 1.0 - hp[2] ** case.step
            d["v"] = ((0.25 + torch.rand(n, generator=gen)) * (sigma * sigma * bc2)).float()
            d["m"] = d["m"] * (1.0 - hp[1] ** case.step)
            d["v"][::7] = 0.0
            d["m"][::7] = 0.0
    d["g"] = g.to(_BF) if case.kernel == "mixed" else g
    d["hp"] = torch.tensor(list(hp) + [0.0] * (8 - len(hp)), dtype=_F32)
    if case.clip is None:
        d["state"] = None
    elif case.clip == "skip":
        d["state"] = torch.tensor([math.inf, 0.0, 1.0, 1.0], dtype=_F32)
    else:
        d["state"] = torch.tensor([2.5, case.clip, 0.0, 0.0], dtype=_F32)
    return d


def _skipped(d) -> bool:
    return d["state"] is not None and float(d["state"][3]) != 0.0


def _scale(d):
    """(the clip scale as the float64 value of its fp32 bits, c)."""
    return (1.0, 0) if d["state"] is None else (float(d["state"][1]), 1)


# ---------------------------------------------------------------------------------------------- oracle and bounds
def _adam_scalars(hp, step):
    """float64 step_size, inv_sqrt_bc2, decay and the bounds e_ss, e_is (relative), d_D (absolute)."""
    lr, b1, b2, eps, wd = (float(x) for x in hp[:5])
    t = step + 1

    def bc(b):
        pw = b ** t
        c = 1.0 - pw
        d_pw = 2 * K_POW * E * pw + TINY
        return c, (d_pw + E * (c + d_pw)) / c

    (c1, e1), (c2, e2) = bc(b1), bc(b2)
    assert e1 < 0.5 and e2 < 0.5
    D = 1.0 - lr * wd
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, ss=lr / c1, e_ss=(1 + E) / (1 - e1) - 1,
                isb2=c2 ** -0.5, e_is=(1 + 2 * K_RSQRT * E) / math.sqrt(1 - e2) - 1,
                D=D, d_D=_gamma(2) * (abs(D) + lr * wd))


def _where64(mask, a, b):
    return torch.where(mask, torch.tensor(a, dtype=_F64), torch.tensor(b, dtype=_F64))


def _decay_mask(kernel, n, decay):
    return torch.arange(n) < decay if kernel != "mixed" else torch.full((n,), bool(decay))


def _adamw_oracle(kernel, d):
    """float64 p, m, v after the step and their bounds (module docstring)."""
    P, M, V = d["p"].double(), d["m"].double(), d["v"].double()
    if _skipped(d):
        z = torch.zeros_like(P)
        return dict(p=P, m=M, v=V), dict(p=z, m=z, v=z)
    s = _adam_scalars(d["hp"], d["step"])
    x = 1 if kernel == "flat" else 0
    scale, c = _scale(d)
    G = d["g"].double() * scale
    b1, b2, eps, ss, isb2, e_ss, e_is = s["b1"], s["b2"], s["eps"], s["ss"], s["isb2"], s["e_ss"], s["e_is"]
    mask = _decay_mask(kernel, P.numel(), d["decay"])
    D, d_D = _where64(mask, s["D"], 1.0), _where64(mask, s["d_D"], 0.0)
    m1 = b1 * M + (1 - b1) * G
    b_m = _gamma(3 + c) * ((b1 * M).abs() + ((1 - b1) * G).abs()) + 3 * TINY
    v1 = b2 * V + (1 - b2) * G * G
    b_v = _gamma(4 + 2 * c) * (b2 * V + (1 - b2) * G * G) + (3 + 2 * G.abs()) * TINY
    sv = v1.sqrt()
    d_sq = torch.minimum(b_v / sv.clamp_min(1e-300), b_v.sqrt())
    d_s = d_sq + E * (sv + d_sq)
    A = sv * isb2
    d_A = d_s * isb2 * (1 + e_is) + A * e_is
    if x:
        d_A = d_A + E * (A + d_A)
    den = A + eps
    d_den = d_A + E * (den + d_A)
    assert bool((d_den < 0.5 * den).all())
    num = ss * m1
    d_num = ss * (1 + e_ss) * b_m + ss * m1.abs() * e_ss
    d_num = d_num + E * (num.abs() + d_num) + TINY
    q = num / den
    d_q0 = (d_num + q.abs() * d_den) / (den - d_den)
    d_q = d_q0 + E * (q.abs() + d_q0) + TINY
    p1 = P * D - q
    b_p = P.abs() * d_D + d_q + E * (q.abs() + d_q) + (1 + x) * E * (1 + E) * ((P * D).abs() + P.abs() * d_D) + TINY
    return dict(p=p1, m=m1, v=v1), dict(p=b_p, m=b_m, v=b_v)


def _sgd_oracle(d, exact=False):
    """float64 p, m after the step and their bounds; ``exact``: bounds of 0 (the power-of-two case)."""
    P, M = d["p"].double(), d["m"].double()
    z = torch.zeros_like(P)
    if _skipped(d):
        return dict(p=P, m=M), dict(p=z, m=z)
    lr, mom, wd, nest, damp = (float(x) for x in d["hp"][:5])
    scale, c = _scale(d)
    Gs = d["g"].double() * scale
    W = _where64(torch.arange(P.numel()) < d["decay"], wd, 0.0)
    gg = Gs + W * P
    Gabs = Gs.abs() + (W * P).abs()
    if d["step"] == 0:
        m1, Mabs, km = gg, Gabs, 2 + c
    else:
        m1, Mabs, km = mom * M + (1 - damp) * gg, (mom * M).abs() + abs(1 - damp) * Gabs, 5 + c
    if nest != 0.0:
        dd, Dabs, kd = gg + mom * m1, Gabs + abs(mom) * Mabs, km + 2
    else:
        dd, Dabs, kd = m1, Mabs, km
    ref = dict(p=P - lr * dd, m=m1)
    if exact:
        return ref, dict(p=z, m=z)
    return ref, dict(p=_gamma(kd + 2) * (P.abs() + abs(lr) * Dabs) + 4 * TINY, m=_gamma(km) * Mabs + 3 * TINY)


def _oracle(case: Case, d):
    if case.kernel == "sgd":
        return _sgd_oracle(d, exact=case.hp == "pow2")
    return _adamw_oracle(case.kernel, d)


@functools.lru_cache(maxsize=None)
def _small_oracle(case: Case):
    return _oracle(case, _small_data(case))


# ------------------------------------------------------------------------------------------------- fp32 emulation
def _fma(a, b, c):
    return (torch.as_tensor(a).double() * torch.as_tensor(b).double() + torch.as_tensor(c).double()).to(_F32)


def _mad(a, b, c, fused):
    return _fma(a, b, c) if fused else a * b + c


def _f(x):
    return torch.tensor(x, dtype=_F32)


def _ulps(x, k):
    """The positive fp32 scalar ``x`` moved by k ulp (zero stays zero): with the rounding of x itself, a result
    within |k| + 1/2 ulp of the exact one."""
    return (x.view(torch.int32) + k).view(_F32) if float(x) >= TINY else x


def _stride(case: Case, wide=False) -> int:
    """Elements one trip of the launch's grid covers."""
    if case.kernel == "sgd":
        return SGD_CAP_ELEMS
    return (case.cap or 2048) * 256 * (8 if wide and case.kernel == "mixed" and case.n % 8 == 0 else 4)


def _emu_adamw(kernel, d, fused, sgn, defect=None, stride=None):
    """The kernel's arithmetic with every operation rounded to fp32.  ``fused``: the contracted form (flat), the form
    of the decay scalar (mixed: adamw_elem itself is always its explicit fmaf form).  pow and rsqrt are float64 rounded
    to fp32 and pushed to their ulp limit, ``sgn`` the direction, each the way that moves the update most.  Defects:
    DEFECTS."""
    hp = d["hp"]
    lr, b1, b2, eps, wd = hp[0], hp[1], hp[2], hp[3], hp[4]
    p, m, v, g0 = d["p"], d["m"], d["v"], d["g"].float()
    out = dict(p=p, m=m, v=v, g=torch.zeros_like(d["g"]))
    if _skipped(d):
        return dict(out, plp=None)
    t = max(d["step"], 1) if defect == "t" else d["step"] + 1
    bc1 = 1 - _ulps(_f(float(b1) ** t), sgn * (K_POW - 1))
    bc2 = 1 - _ulps(_f(float(b2) ** t), -sgn * (K_POW - 1))
    if defect == "bc2":
        bc2 = bc2 * _f(1 + 1e-4)
    ss = lr / bc1
    isb2 = _ulps((bc2.double() ** -0.5).to(_F32), -sgn * (K_RSQRT - 1))
    elem_fused = fused or kernel == "mixed"
    n = p.numel()
    nd = d["decay"] + (dict(decay_past=4, decay_short=-4).get(defect, 0) if kernel == "flat" else 0)
    mask = _decay_mask(kernel, n, nd)
    g = g0 * d["state"][1] if d["state"] is not None else g0
    if defect == "coupled":
        g = g + torch.where(mask, wd * p, _f(0.0))
        dec = torch.ones_like(p)
    else:
        dec = torch.where(mask, _fma(-lr, wd, 1.0) if fused else 1 - lr * wd, _f(1.0))
    B1, B2 = (b2, b1) if defect == "betas" else (b1, b2)
    m1 = _mad(B1, m, (1 - B1) * g, elem_fused)
    v1 = _mad(B2, v, ((1 - B2) * g) * g, elem_fused)
    sv = v1.sqrt()
    if defect == "eps_before":
        den = (sv + eps) * isb2
    elif defect == "eps_inside":
        den = (v1 + eps).sqrt() * isb2
    else:
        den = _mad(sv, isb2, eps, elem_fused)
    q = (ss * m1) / den
    p1 = _fma(p, dec, -q) if elem_fused else p * dec - q
    out = dict(p=p1, m=m1, v=v1, g=out["g"])
    if defect == "tail":
        keep = torch.arange(n) < (n // stride) * stride
        out = dict(p=torch.where(keep, p1, p), m=torch.where(keep, m1, m), v=torch.where(keep, v1, v),
                   g=torch.where(keep, out["g"], d["g"]))
    out["plp"] = _trunc(out["p"]) if defect == "trunc" else out["p"].to(_BF)
    return out


def _emu_sgd(d, fused, defect=None, stride=None):
    hp = d["hp"]
    lr, mom, wd, nest, damp = hp[0], hp[1], hp[2], float(hp[3]) != 0.0, hp[4]
    p, m, g = d["p"], d["m"], d["g"]
    if _skipped(d):
        return dict(p=p, m=m, g=torch.zeros_like(g))
    n = p.numel()
    nd = d["decay"] + dict(decay_past=4, decay_short=-4).get(defect, 0)
    w = torch.where(torch.arange(n) < nd, wd, _f(0.0))
    clip = d["state"] is not None
    if clip and defect == "clip_after":
        gg = (g + w * p) * d["state"][1]
    else:
        gg = _mad(w, p, g * d["state"][1] if clip else g, fused)
    omd = 1 - damp
    if d["step"] == 0:
        m1 = omd * gg if defect == "damp_first" else gg
    else:
        m1 = _mad(mom, m, omd * gg, fused)
    dd = _mad(mom, m if defect == "nesterov_old" else m1, gg, fused) if nest else m1
    p1 = _fma(-lr, dd, p) if fused else p - lr * dd
    out = dict(p=p1, m=m1, g=torch.zeros_like(g))
    if defect == "tail":
        keep = torch.arange(n) < (n // stride) * stride
        out = dict(p=torch.where(keep, p1, p), m=torch.where(keep, m1, m), g=torch.where(keep, out["g"], g))
    return out


def _variants(kernel):
    return [(f,) for f in (False, True)] if kernel == "sgd" else [(f, s) for f in (False, True) for s in (1, -1)]


def _emulate(case: Case, d, variant, defect=None, wide=False):
    if case.kernel == "sgd":
        return _emu_sgd(d, *variant, defect=defect, stride=_stride(case))
    return _emu_adamw(case.kernel, d, *variant, defect=defect, stride=_stride(case, wide))


def _ratios(case: Case, d, out, ref, bound):
    """The ratio of every output: p, m, v against their bounds; g: inf unless all zero bits; plp: inf unless it is the
    round-to-nearest-even of this very p (after a skipped step: unless untouched, which is None here)."""
    r = {k: _ratio(out[k], ref[k], bound[k]) for k in ref}
    r["g"] = 0.0 if bool((_bits(out["g"]) == 0).all()) else math.inf
    if case.kernel == "mixed" and not _skipped(d):
        r["plp"] = 0.0 if _same_bits(out["plp"], out["p"].to(_BF)) else math.inf
    return r


def _exact_properties(case: Case, d, out):
    """Section 5's exact cases, on whichever outputs (emulation or GPU) are given."""
    if case.kernel == "sgd":
        return
    hp = ADAM_HPS[case.hp]
    if _skipped(d):
        assert all(_same_bits(out[k], d[k]) for k in ("p", "m", "v")), "a skipped step changes nothing"
        return
    if hp[1] == 0.0 and case.clip in (None, 1.0):
        assert _same_bits(out["m"], d["g"].float() + 0.0), "b1 = 0: m == g"
    if hp[0] == 0.0:
        assert _same_bits(out["p"], d["p"]), "lr = 0: p unchanged"
    elif case.step == 0:                                        # m = v = 0: where g = 0, p is p times the decay
        z = d["g"].float() == 0
        lr, wd = d["hp"][0], d["hp"][4]
        mask = _decay_mask(case.kernel, case.n, case.decay)
        want = [d["p"] * torch.where(mask, dec, _f(1.0)) for dec in (1 - lr * wd, _fma(-lr, wd, 1.0))]
        assert bool(z.any()) or case.n <= 12
        assert any(torch.equal(out["p"][z], w[z]) for w in want), "g = m = v = 0: p' = fl(p decay)"
        assert bool((out["m"][z] == 0).all()) and bool((out["v"][z] == 0).all())


def _say(where, case, r):
    name = dict(sgd="sgd_flat", flat="adamw_flat", mixed="adamw_mixed")[case.kernel]
    for k, x in r.items():
        print(f"OPTIM_{where} {name} {k} {_cid(case)} {x:.3f}")


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_emulation_stays_inside_the_bound(case):
    """The check that the bounds are not too tight: the fp32 emulation, contracted and not, pow and rsqrt at their
    ulp limits in either direction, on every case the GPU tests use."""
    d = _data(case) if case.n >= 100_000 else _small_data(case)
    ref, bound = _oracle(case, d) if case.n >= 100_000 else _small_oracle(case)
    worst = {}
    for variant in _variants(case.kernel):
        out = _emulate(case, d, variant)
        _exact_properties(case, d, out)
        for k, x in _ratios(case, d, out, ref, bound).items():
            worst[k] = max(worst.get(k, 0.0), x)
    _say("EMU", case, worst)
    assert all(x <= 1.0 for x in worst.values()), worst


# ------------------------------------------------------------------------------------------------ injected defects
# One table for the defect tests and the old-tolerance record.  ``cases``: per kernel, the named case on which the
# defect must exceed 1.0 in one of ``outs``.  ``old``: per kernel, whether the emulation with the defect passes
# assert_close(p, ref, rtol=1e-5, atol=1e-6) on the old tests' inputs (test_old_tolerance_misses_the_recorded_defects).
Defect = namedtuple("Defect", "num key what cases outs old")
_F9 = Case("flat", 4104, "torch", 9, "randn", 1028, None, None)
_M9 = Case("mixed", 4104, "torch", 9, "randn", 1, None, None)
_FE = Case("flat", 4104, "eps3", 9, "small4", 4104, None, None)
_ME = Case("mixed", 4104, "eps3", 9, "small4", 1, None, None)
_S5 = Case("sgd", 4104, "nest", 5, "randn", 1028, None, None)
DEFECTS = [
    Defect(1, "t", "bias correction with t instead of t + 1 (after the first step)",
           dict(flat=_F9, mixed=_M9), ("p",), dict(flat=False, mixed=False)),
    Defect(2, "eps_before", "eps added before the inv_sqrt_bc2 scaling",
           dict(flat=_FE, mixed=_ME), ("p",), dict(flat=True, mixed=True)),
    Defect(3, "eps_inside", "eps added inside the square root",
           dict(flat=_FE, mixed=_ME), ("p",), dict(flat=False, mixed=False)),
    Defect(4, "coupled", "weight decay coupled into the gradient instead of decoupled",
           dict(flat=_F9, mixed=_M9), ("p", "m", "v"), dict(flat=False, mixed=False)),
    Defect(5, "decay_past", "weight decay applied one float4 past n_decay",
           dict(flat=_F9, sgd=_S5), ("p",), dict(flat=False, sgd=False)),
    Defect(5, "decay_short", "weight decay applied one float4 short of n_decay",
           dict(flat=_F9, sgd=_S5), ("p",), dict(flat=False, sgd=False)),
    Defect(6, "betas", "m and v updated with each other's beta",
           dict(flat=_F9, mixed=_M9), ("m", "v"), dict(flat=False, mixed=False)),
    Defect(7, "trunc", "plp truncated instead of rounded to nearest even",
           dict(mixed=_M9), ("plp",), dict(mixed=False)),
    Defect(8, "clip_after", "clip scale applied after weight decay",
           dict(sgd=Case("sgd", 4104, "nest", 5, "randn", 1028, 0.37, None)), ("p", "m"), dict(sgd=False)),
    Defect(9, "damp_first", "dampening applied on the first step",
           dict(sgd=Case("sgd", 4104, "nest", 0, "randn", 1028, 1.0, None)), ("p", "m"), dict(sgd=False)),
    Defect(10, "nesterov_old", "Nesterov using the old momentum", dict(sgd=_S5), ("p",), dict(sgd=False)),
    Defect(11, "tail", "the last partial grid-stride trip dropped",
           dict(flat=Case("flat", N_CAP4, "gpt2", 9, "randn", N_CAP4 - 4, None, 2),
                mixed=Case("mixed", N_CAP4, "gpt2", 9, "randn", 1, None, 2),
                sgd=Case("sgd", N_BIG, "nest", 3, "randn", N_BIG - 4, 0.37, None)),
           ("p", "m", "g"), dict(flat=False, mixed=False, sgd=False)),
    # At t = 1 ... 10 the cancellation in 1 - 0.999^t at pow's 16 ulp honestly allows 2e-3 ... 2e-4 of bc2; at
    # t = 10^3 it allows 19 E and from t = 10^5 on nothing: there a relative 1e-4 is far outside
    Defect(12, "bc2", "bc2 taken with a relative error of 1e-4",
           dict(flat=Case("flat", 4100, "torch", 99_999, "log", 4100, None, None),
                mixed=Case("mixed", 4100, "torch", 9_999_999, "log", 1, None, None)),
           ("p",), dict(flat=True, mixed=True)),
]
_DEFECT_RUNS = [(x, k) for x in DEFECTS for k in x.cases]


@pytest.mark.parametrize("defect,kernel", _DEFECT_RUNS, ids=[f"{x.num}-{x.key}-{k}" for x, k in _DEFECT_RUNS])
def test_injected_defect_exceeds_the_bound(defect, kernel):
    """Each defect, injected into every variant of the emulation, is outside a bound on its named case -- a case of
    the GPU tests -- while the emulation without it is inside (test_emulation_stays_inside_the_bound)."""
    case = defect.cases[kernel]
    assert case in CASES and case.kernel == kernel
    big = case.n >= 100_000
    d = _data(case) if big else _small_data(case)
    ref, bound = _oracle(case, d) if big else _small_oracle(case)
    for variant in _variants(kernel):
        for wide in ((False, True) if defect.key == "tail" and kernel == "mixed" else (False,)):
            r = _ratios(case, d, _emulate(case, d, variant, defect.key, wide), ref, bound)
            print(f"{defect.num} {defect.key} {_cid(case)} {variant}:", " ".join(f"{k}={x:.3g}" for k, x in r.items()))
            assert max(r[k] for k in defect.outs if k in r) > 1.0, r


def _old_accepts(got, ref, rtol=1e-5, atol=1e-6) -> bool:
    """torch.testing.assert_close's criterion."""
    return bool(((got.double() - ref).abs() <= atol + rtol * ref.abs()).all())


def _old_inputs(kernel):
    """The inputs of the old tests: test_adamw_flat_matches_torch and test_adamw_mixed_matches_torch (three steps from
    m = v = 0, randn p and gradients), test_sgd_flat_matches_reference (one step, first or not, Nesterov or not;
    with the clip state of test_gpu_grad_clip.py's scale for the clip defect).  Yields (case, data, gradients)."""
    gen = _gen("old", kernel)
    if kernel == "sgd":
        n, n_decay = 4096 * 37 + 4, 4096 * 20
        for first in (0, 5):
            for nesterov in (0.0, 1.0):
                for clip in (None, 0.37):
                    case = Case("sgd", n, "old", first, "randn", n_decay, clip, None)
                    d = dict(step=first, decay=n_decay, p=torch.randn(n, generator=gen),
                             m=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen),
                             hp=torch.tensor([0.1, 0.9, 1e-3, nesterov, 0.1, 0, 0, 0], dtype=_F32),
                             state=None if clip is None else torch.tensor([2.5, clip, 0.0, 0.0], dtype=_F32))
                    yield case, d, [d["g"]]
        return
    n, decay, hp = (8192, 4096, [1e-3, 0.9, 0.999, 1e-8, 0.01]) if kernel == "flat" else \
        (4096 * 9 + 4, 1, [1e-3, 0.9, 0.95, 1e-8, 0.1])
    case = Case(kernel, n, "old", 0, "randn", decay, None, None)
    d = dict(step=0, decay=decay, p=torch.randn(n, generator=gen), m=torch.zeros(n), v=torch.zeros(n), state=None,
             hp=torch.tensor(hp + [0, 0, 0], dtype=_F32))
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    yield case, d, [g.to(_BF) for g in grads] if kernel == "mixed" else grads


def _old_run(kernel, key):
    """(accepted by the old tolerance, largest bound ratio over the steps) of the emulation with defect ``key``."""
    accepted, worst = True, 0.0
    for case, d, grads in _old_inputs(kernel):
        if key == "clip_after" and case.clip is None:
            continue
        d64 = dict(d)                                           # the float64 chain the old test's reference stands for
        for i, g in enumerate(grads):
            d = dict(d, g=g, step=d["step"] + (i > 0))
            d64 = dict(d64, g=g, step=d["step"])
            ref, bound = _oracle(case, d)                       # this step, from the state the emulation is in
            out = _emulate(case, d, _variants(kernel)[0], key)
            worst = max(worst, max(_ratios(case, d, out, ref, bound).values()))
            d = dict(d, **{k: out[k] for k in ref})
            chain, _ = _oracle(case, d64)
            d64 = dict(d64, **chain)
        accepted = accepted and _old_accepts(out["p"], d64["p"])
        if kernel == "sgd":
            accepted = accepted and _old_accepts(out["m"], d64["m"])
        accepted = accepted and bool((out["g"].float() == 0).all())
        if kernel == "mixed":                                   # the old test asserts plp == bf16(p) too
            accepted = accepted and _same_bits(out["plp"], out["p"].to(_BF))
    return accepted, worst


def test_old_tolerance_misses_the_recorded_defects():
    """What the old tolerance lets through, kept on record: on the inputs and the tolerance of the old tests (float64
    standing in for their fp32 torch.optim reference) the emulation without a defect passes and is inside every bound,
    and of DEFECTS the old tolerance accepts exactly those whose ``old`` entry says so: eps added before the
    inv_sqrt_bc2 scaling, and bc2 off by a relative 1e-4, in both AdamW kernels.  Both are outside a bound on those
    same inputs, but for bc2 in the flat kernel: with b2 = 0.999 and t <= 3 the cancellation at pow's 16 ulp allows
    that much, and its named case is t = 10^5.  Rejected by the old tolerance too, through p after three steps (m
    and v themselves were never compared): the bias correction with t for t + 1 (its second step is 34 % off), eps
    inside the root, coupled decay, the decay boundary off by one float4 (lr wd |p| = 1e-5 |p| three times over
    against rtol = 1e-5), swapped betas, the truncated plp, the SGD defects, and the dropped partial trip -- there
    only because the one trip those inputs take is itself partial; a second trip they never take."""
    for kernel in ("sgd", "flat", "mixed"):
        ok, r0 = _old_run(kernel, None)
        print(f"{kernel} without a defect: accepted={ok} bound ratio {r0:.3f}")
        assert ok and r0 <= 1.0
    for x in DEFECTS:
        for kernel, want in x.old.items():
            ok, r = _old_run(kernel, x.key)
            print(f"{x.num} {x.key} {kernel}: passes assert_close={ok}, bound ratio {r:.3g}")
            assert ok == want, (x.key, kernel)
            if ok and (x.key, kernel) != ("bc2", "flat"):
                assert r > 1.0, (x.key, kernel)


def test_case_set_covers_what_the_issue_names():
    for k in ("flat", "mixed", "sgd"):
        assert {c.n for c in CASES if c.kernel == k} >= set(SIZES)
    for k in ("flat", "mixed"):
        assert {c.step for c in CASES if c.kernel == k} >= set(STEPS)
        assert {c.hp for c in CASES if c.kernel == k} == set(ADAM_HPS)
        assert {c.clip for c in CASES if c.kernel == k} == {None, 1.0, 0.37, "skip"}
        assert any(c.cap == 2 and c.n == N_CAP4 for c in CASES if c.kernel == k)
    assert any(c.cap == 2 and c.n == N_CAP8 and c.kernel == "mixed" for c in CASES)
    assert {c.decay for c in CASES if c.kernel == "flat" and c.n == 4104} >= {0, 4, 1028, 4100, 4104}
    assert {c.decay for c in CASES if c.kernel == "mixed"} == {0, 1}
    assert N_BIG == 2048 * 256 * 4 + 1028 and any(c.n == N_BIG for c in CASES)
    g = _bf16_sweep()
    assert g.numel() == 768 and bool((g.float().abs() < TINY).sum() == 128) and bool(g.isfinite().all())
    # where b^t leaves fp32: the figures of the docstring
    for b, normal, gone in ((0.9, 829, 987), (0.95, 1703, 2028), (0.999, 87294, 103922)):
        b = float(_f(b))
        assert b ** (normal - 1) >= TINY > b ** normal and b ** (gone - 1) >= 2.0 ** -150 > b ** gone


# --------------------------------------------------------------------------------------------------- GPU: plumbing
def _lib():
    from polyaxon_amd.ops import _native

    return _native.lib("plx_train")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _Guarded:
    """Device buffers between guard words: PAD words of a fixed pattern on both sides of each."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def put(self, name, t, pad=PAD):
        it, pat = (torch.int16, GUARD16) if t.dtype == _BF else (torch.int32, GUARD32)
        n = t.numel()
        buf = torch.full((pad + n + pad,), pat, dtype=it, device=self.dev)
        buf[pad:pad + n].copy_(t.contiguous().view(it))
        self.bufs[name] = (buf, pad, n, t.dtype, pat)
        return buf[pad:pad + n].data_ptr()

    def get(self, name):
        buf, pad, n, dtype, _ = self.bufs[name]
        return buf[pad:pad + n].cpu().view(dtype)

    def broken(self):
        return [k for k, (buf, pad, n, _, pat) in self.bufs.items()
                if not (bool((buf[:pad] == pat).all()) and bool((buf[pad + n:] == pat).all()))]


def _unwritten(n):
    return torch.full((n,), GUARD16, dtype=torch.int16).view(_BF)


def _launch(dev, case: Case, d, wide=0, clip_entry=None, pads=None):
    """One launch through the C entry point on guarded copies of ``d``; the buffers afterwards, on the host.
    ``clip_entry``: False forces the entry point without clipping.  ``pads``: guard words per buffer (an odd multiple
    of 4 bf16 elements leaves that pointer 8-byte aligned only)."""
    lib, b = _lib(), _Guarded(dev)
    pads = pads or {}
    names = ["p", "g", "m"] + (["v"] if case.kernel != "sgd" else [])
    ptr = {k: b.put(k, d[k], pads.get(k, PAD)) for k in names}
    if case.kernel == "mixed":
        ptr["plp"] = b.put("plp", _unwritten(case.n), pads.get("plp", PAD))
    ptr["hp"] = b.put("hp", d["hp"])
    ptr["step"] = b.put("step", torch.tensor([d["step"]], dtype=torch.int32))
    clip = d["state"] is not None if clip_entry is None else clip_entry
    tail = (b.put("state", d["state"]),) if clip else ()
    st = _stream(dev)
    try:
        lib.plx_set_adamw_grid_cap(case.cap or 2048)
        lib.plx_set_adamw_wide(wide)
        if case.kernel == "sgd":
            fn = lib.plx_sgd_flat_clip if clip else lib.plx_sgd_flat
            rc = fn(ptr["p"], ptr["g"], ptr["m"], case.n, d["decay"], ptr["hp"], ptr["step"], *tail, st)
        elif case.kernel == "flat":
            fn = lib.plx_adamw_flat_clip if clip else lib.plx_adamw_flat
            rc = fn(ptr["p"], ptr["g"], ptr["m"], ptr["v"], case.n, d["decay"], ptr["hp"], ptr["step"], *tail, st)
        else:
            fn = lib.plx_adamw_mixed_clip if clip else lib.plx_adamw_mixed
            rc = fn(ptr["p"], ptr["g"], ptr["m"], ptr["v"], ptr["plp"], case.n, d["decay"], ptr["hp"], ptr["step"],
                    *tail, st)
        torch.cuda.synchronize(dev)
    finally:
        lib.plx_set_adamw_grid_cap(2048)        # the library defaults, which is what every other test runs with
        lib.plx_set_adamw_wide(0)
    assert rc == 0
    assert not b.broken(), "guard words"
    out = {k: b.get(k) for k in b.bufs}
    assert _same_bits(out["hp"], d["hp"]) and int(out["step"]) == d["step"]
    assert not clip or _same_bits(out["state"], d["state"])
    return out


def _check_gpu(case: Case, d, out, ref, bound):
    r = _ratios(case, d, out, ref, bound)
    _say("RATIO", case, r)
    assert all(x <= 1.0 for x in r.values()), r
    _exact_properties(case, d, out)
    if case.kernel == "mixed" and _skipped(d):
        assert _same_bits(out["plp"], _unwritten(case.n)), "a skipped step leaves plp alone"


GPU_SMALL = [c for c in SMALL if c.kernel != "mixed"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_SMALL, ids=_cid)
def test_sgd_and_adamw_flat_within_bound(cuda, case):
    """p, m (and v) against their bounds, g all zero bits, guards intact, hp / step / state unchanged; a clip scale
    of 1.0 bit for bit the entry point without clipping."""
    d = _small_data(case)
    out = _launch(cuda, case, d)
    _check_gpu(case, d, out, *_small_oracle(case))
    if case.clip == 1.0:
        plain = _launch(cuda, case, d, clip_entry=False)
        assert all(_same_bits(out[k], plain[k]) for k in ("p", "g", "m") + (("v",) if case.kernel == "flat" else ()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in SMALL if c.kernel == "mixed"], ids=_cid)
def test_adamw_mixed_within_bound_and_paths_agree(cuda, case):
    """The 4-wide kernel against the bounds; the 8-wide non-temporal and plain ones (taken when n % 8 == 0) bit for
    bit the same p, m, v, plp, g; with g and plp on pointers that are only 8-byte aligned the knob falls back to the
    4-wide kernel: the same bits again.  plp is bf16_rne of the kernel's own p and plx_cast_lp reproduces it."""
    d = _small_data(case)
    ref, bound = _small_oracle(case)
    out = _launch(cuda, case, d)
    _check_gpu(case, d, out, ref, bound)
    keys = ("p", "g", "m", "v", "plp")
    for wide in (1, 2):
        other = _launch(cuda, case, d, wide=wide)
        assert all(_same_bits(out[k], other[k]) for k in keys), wide
    assert (PAD + 4) * 2 % 16 == 8
    for wide in (0, 1):
        other = _launch(cuda, case, d, wide=wide, pads=dict(g=PAD + 4, plp=PAD + 4))
        assert all(_same_bits(out[k], other[k]) for k in keys), ("8-byte aligned", wide)
    if case.clip == 1.0:
        for wide in (0, 1):
            plain = _launch(cuda, case, d, wide=wide, clip_entry=False)
            assert all(_same_bits(out[k], plain[k]) for k in keys), ("scale 1.0", wide)
    if not _skipped(d):
        assert _same_bits(_cast_lp(cuda, out["p"]), out["plp"])


def _cast_lp(dev, p):
    b = _Guarded(dev)
    src, dst = b.put("p", p), b.put("plp", _unwritten(p.numel()))
    assert _lib().plx_cast_lp(src, dst, p.numel(), _stream(dev)) == 0
    torch.cuda.synchronize(dev)
    assert not b.broken(), "guard words"
    assert _same_bits(b.get("p"), p)
    return b.get("plp")


@pytest.mark.gpu
def test_sgd_and_cast_lp_above_their_grid_cap(cuda):
    """n = 2048 * 256 * 4 + 1028: one full trip of the fixed 2048-block grid and a ragged second one.  cast_lp on
    fp32 values that include every tie (low half 0x8000, even and odd upper half), subnormals and both infinities."""
    case = next(c for c in CASES if c.n == N_BIG)
    d = _data(case)
    ref, bound = _oracle(case, d)
    _check_gpu(case, d, _launch(cuda, case, d), ref, bound)
    gen = _gen("cast")
    bits = torch.randint(-2 ** 31, 2 ** 31, (N_BIG,), generator=gen, dtype=torch.int64).to(torch.int32)
    bits[::3] = (bits[::3] & -65536) | 0x8000                      # ties
    bits[1::64] &= ~0x7F800000                                     # subnormals and zeros
    p = bits.view(_F32).clone()
    p[p.isnan()] = math.inf
    p[-1028:-1024] = torch.tensor([math.inf, -math.inf, 0.0, -0.0])
    assert _same_bits(_cast_lp(cuda, p), p.to(_BF))
    assert not _same_bits(_trunc(p), p.to(_BF))


def test_cast_reference_rounds_to_nearest_even():
    """The reference of every plp assertion: torch's fp32 -> bf16 on the host is round-to-nearest-even."""
    x = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x00008000, 0x00018000],
                     dtype=torch.int32).view(_F32)
    want = torch.tensor([0x3F80, 0x3F82, 0x3F81, 0x3F80, 0x0000, 0x0002], dtype=torch.int16)
    assert torch.equal(x.to(_BF).view(torch.int16), want)


# ------------------------------------------------------------------------------------------ GPU: argument validation
@pytest.mark.gpu
def test_refused_arguments_launch_nothing(cuda):
    """What the entry points refuse before launching returns 1 and leaves every buffer bit-unchanged: n or n_decay
    not a multiple of 4, a null clip state at a _clip entry point, and -- added with this test -- a negative n and
    what the kernels would have dereferenced: a null hp or step, a null buffer with n > 0.  No call here passes a
    pointer or size a launched kernel could take out of range."""
    lib, st, b = _lib(), _stream(cuda), _Guarded(cuda)
    n = 64
    gen = _gen("args")
    host = dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen), m=torch.randn(n, generator=gen),
                v=torch.rand(n, generator=gen), gb=torch.randn(n, generator=gen).to(_BF), plp=_unwritten(n),
                hp=torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 0, 0], dtype=_F32),
                step=torch.tensor([3], dtype=torch.int32), state=torch.tensor([2.5, 0.37, 0.0, 0.0], dtype=_F32))
    a = {k: b.put(k, t) for k, t in host.items()}
    P, G, M, V, GB, L, HP, ST, CS = (a[k] for k in ("p", "g", "m", "v", "gb", "plp", "hp", "step", "state"))

    def sgd(p=P, g=G, m=M, n=n, nd=n, hp=HP):
        return [lib.plx_sgd_flat(p, g, m, n, nd, hp, ST, st), lib.plx_sgd_flat_clip(p, g, m, n, nd, hp, ST, CS, st)]

    def flat(p=P, g=G, m=M, v=V, n=n, nd=n, hp=HP, step=ST):
        return [lib.plx_adamw_flat(p, g, m, v, n, nd, hp, step, st),
                lib.plx_adamw_flat_clip(p, g, m, v, n, nd, hp, step, CS, st)]

    def mixed(p=P, g=GB, m=M, v=V, plp=L, n=n, hp=HP, step=ST):
        return [lib.plx_adamw_mixed(p, g, m, v, plp, n, 1, hp, step, st),
                lib.plx_adamw_mixed_clip(p, g, m, v, plp, n, 1, hp, step, CS, st)]

    rcs = []
    for bad in (dict(n=62), dict(n=63), dict(n=-4), dict(n=-64), dict(hp=None), dict(p=None), dict(g=None),
                dict(m=None)):
        rcs += sgd(**bad) + flat(**bad) + mixed(**bad)
    for bad in (dict(nd=6), dict(nd=61)):
        rcs += sgd(**bad) + flat(**bad)
    for bad in (dict(v=None), dict(step=None)):
        rcs += flat(**bad) + mixed(**bad)
    rcs += mixed(plp=None)
    rcs += [lib.plx_sgd_flat_clip(P, G, M, n, n, HP, ST, None, st),
            lib.plx_adamw_flat_clip(P, G, M, V, n, n, HP, ST, None, st),
            lib.plx_adamw_mixed_clip(P, GB, M, V, L, n, 1, HP, ST, None, st)]
    rcs += [lib.plx_cast_lp(P, L, 62, st), lib.plx_cast_lp(P, L, -4, st), lib.plx_cast_lp(None, L, n, st),
            lib.plx_cast_lp(P, None, n, st)]
    torch.cuda.synchronize(cuda)
    assert rcs and all(rc == 1 for rc in rcs), rcs
    assert not b.broken() and all(_same_bits(b.get(k), t) for k, t in host.items())
    # the same buffers with good arguments are accepted (a null first_step of SGD means: never a first step)
    assert lib.plx_sgd_flat(P, G, M, n, n, HP, None, st) == 0
    assert flat() == [0, 0] and mixed() == [0, 0] and lib.plx_cast_lp(P, L, n, st) == 0
    assert sgd(n=0) == [0, 0] and flat(n=0) == [0, 0] and mixed(n=0) == [0, 0]
    torch.cuda.synchronize(cuda)
    assert not b.broken() and not _same_bits(b.get("p"), host["p"]) and not _same_bits(b.get("plp"), host["plp"])
    assert bool((b.get("g") == 0).all()) and bool((b.get("gb").float() == 0).all())
