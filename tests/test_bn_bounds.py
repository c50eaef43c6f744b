"""BatchNorm (csrc/bn_kernels.hip) against an fp64 reference with an a-priori, per-element bound.

tests/test_gpu_bn.py judges these kernels by assert_close at 2e-2 .. 3e-2 on zero-mean Gaussian data, and the equality
tests compare one kernel of the file with another.  Here every output of plx_bn_forward / plx_bn_backward, of the two
apply entry points and of the stem's plx_stem_bn_pool_forward / _backward is held to a bound derived from the dataflow
in the source (`:n` cites a line of csrc/bn_kernels.hip).  Vocabulary of test_norm_bounds.py / test_conv_bounds.py:
U = 2^-8 at a bf16 store, E = 2^-24 per fp32 rounding, gamma(k) = kE / (1 - kE) times the sum of ABSOLUTE values for
a chain of k fp32 additions, the statistic max |got - ref| / bound, the assertion <= 1.0.  Nothing is excluded: the
oracle of a pass takes as inputs what that pass reads (the scale / bias, mean / invstd and ReLU mask the kernel stored,
each checked on its own; window positions the test hands over), so no element is "near a threshold".

Derivation, one paragraph per quantity (names as in the BN_RATIO lines):

l1s, l1q   level-1 partials of bn_stats_kernel, read back from the workspace.  d = fl(x - x[0]) (:84) is one rounding,
           s += d a chain of rows_per_block / R additions per thread (:79) plus the R - 1 of the LDS combine (:96):
           gamma(chain + 1) * sum |d| per block; q = fmaf(d, d, q) carries d's rounding twice and the fma's:
           gamma(chain + 3) * sum d^2.  The shift is row 0, so a row 0 that is an outlier (kind row0out) pays through
           sum |d|, not through an exemption.
l1a, l1b   bn_bwd_reduce_kernel (:464-465), the stem's pass 1 (:866-867, chain 4 pixels per quad row + 256 / G LDS
           additions, :888) and, as rpa / rpb, the ResBn partials of the dx pass (:566-568, chain = grid-stride trips
           + 256 / G - 1): gamma(chain) * sum |dz| and gamma(chain + 3) * sum |dz * xhat| (xhat = fl(fl(x - mu) * is):
           two roundings, and the fma's).
level 2    l1_rows<1024> (:124) adds 4 rows per thread, the combine (:153, :303) 16 groups: 20 more additions on the
           same sums of absolute values.  fin_sum2 (:165) is fp64 and is charged nothing.  External partials are inputs:
           only these 20 are charged, on sum |partial|.
mean       m = S / M in fp64 on the fp32 sums, mean = shift + (float)m (:239): dS / M + E |m|, then E |mean|.
invstd     var = Q / M - m^2 in fp64 (:237): |d var| <= dQ / M + 2 |m| dS / M + (dS / M)^2; (float)var + eps (:240) two
           roundings relative to var + eps; rsqrtf at half the relative error, plus 2 ulp (RSQ).  With unshifted
           external partials and a large mean (kind off300, ext) the cancellation Q / M - m^2 is paid through dQ, dS.
scale,bias g * invstd (:244) one rounding; bias = beta - mean * g * invstd (:245): the product's error is absolute
           (|g| (|mean| d_is + is d_mean) + 3E |P|), so a beta that cancels it does not shrink it.
rmean,rvar (1 - mom) * r + mom * stat (:248-249): 3E on each term; the unbiased variance (float)(var * M / (M - 1))
           carries d var * M / (M - 1).
y          apply (:406-415): fmaf(x, a, b), with a residual fmaf(res, ra, rb) (exact without res_sb) and one fp32
           addition, then U at the store; ReLU is 1-Lipschitz.  mask: the bit must equal y > 0 of the stored y.
dbeta,     (float) of the fp64 totals: the sums' bounds + E; accumulate adds one rounding of the sum (:261).
dgamma
cA,cB,cD   k1 = g * is, k2 = db / M, k3 = dg / M (:263-264; a division is charged 2.5 ulp), A = k1, B = -k1 k3 is
           (:267), D = -k1 k2 + k1 k3 is mean (:268): D's terms cancel when the mean is large, so it is charged
           |k1| d_k2 + |k1 is mean| d_k3 + 6E (|k1 k2| + |k1 k3 is mean|).
dx         fmaf(A, dz, fmaf(B, x, D)) (:573, :864, :1140) from the coefficients the kernel stored: E |B x + D|,
           E |dx|, U at the store.  dxt is the same output against the textbook k1 (dz - k2 - xhat k3) from the true
           sums, its bound widened by |dz| d_A + |x| d_B + d_D.  dres = bf16(dz) from bf16: bit-exact.
stem       sy / sidx: the pooled y and the window positions must equal BIT FOR BIT the pool (first maximum in
           (kh, kw) order) of bf16(relu(fmaf(x, a, b))) with _fma a true fma (x * a exact in fp64, TwoSum, and the
           error's sign where the fp64 sum lies on an fp32 tie; test_fma_is_a_true_fused_multiply_add checks it against
           fractions).  sy is also held to U |y| + E-terms against fp64.  The backward's dz is the gather by position in
           the kernel's window order (IEEE fp32 additions), rounded to bf16 and masked by the pixel's own fmaf > 0.
exact      test_gpu_exact_data_gives_exact_outputs: small-integer x and dy, power-of-two gamma / invstd, integer mean,
           M a power of two: every sum is an exact fp32 number in any order and mean, the running statistics, dgamma,
           dbeta, the coefficients and dx must match exactly (invstd to rsqrtf's 2 ulp).

Largest measured ratio per family on an MI355X (BN_RATIO lines of the GPU cases; the fp32 emulation's over the
CPU-sized cases in brackets).  own: the call runs its statistics / reduce pass; ext: external partials; stem: the stem
entry points (thinned kernels and predecessors give identical figures):

    family  mean           invstd         scale          bias           rmean          rvar           y / sy
    own     0.789 (0.789)  0.184 (0.140)  0.313 (0.279)  0.335 (0.335)  0.565 (0.565)  0.631 (0.631)  0.996 (0.996)
    ext     0.038 (0.038)  0.148 (0.105)  0.140 (0.108)  0.056 (0.068)  0.178 (0.178)  0.152 (0.152)  0.996 (0.996)
    stem    0.041 (0.041)  0.111 (0.111)  0.104 (0.104)  0.293 (0.293)  0.204 (0.204)  0.176 (0.176)  0.996 (0.996)

    family  l1s            l1q            l1a            l1b            rpa            rpb
    own     0.220 (0.126)  0.525 (0.512)  0.077 (0.077)  0.286 (0.286)  0.187 (0.019)  0.701 (0.701)
    stem    0.060 (0.060)  0.511 (0.511)  0.001 (0.000)  0.329 (0.329)  -              -

    family  dbeta          dgamma         cA             cB             cD             dx             dxt
    own     0.302 (0.302)  0.574 (0.584)  0.996 (0.996)  0.085 (0.085)  0.088 (0.088)  0.996 (0.996)  0.996 (0.996)
    ext     0.035 (0.035)  0.191 (0.191)  0.971 (0.971)  0.162 (0.162)  0.101 (0.101)  0.996 (0.996)  0.996 (0.996)
    stem    0.000 (0.000)  0.086 (0.086)  0.976 (0.978)  0.106 (0.106)  0.046 (0.050)  0.996 (0.995)  0.994 (0.994)

    apply entry points (plx_bn_apply, plx_bn_apply_res_relu): y 0.996.  Autograd path (bn_act, defer_apply +
    residual_link): y 0.994, dx of both inputs 0.996, statistics and parameter gradients 0.01 .. 0.30, ResBn partials
    rpb 0.070.  mask, dres, sidx and the stem's y bits: exact everywhere.  (The emulation does not run the cases above
    2^21 elements, hence the smaller l1s / rpa / invstd in brackets.)

y, dx, dxt, sy and cA sit at the rounding itself (one U, one E).  The fp32 sums use a few percent to a half of bounds
that are worst case in every sign.  Below 0.05: ext mean / dbeta (20 additions charged at full sign-coherent weight on
partials of random sign; kind posg loads dbeta to 0.035), and l1a / dbeta of the stem, where dz holds bf16 values of
similar exponent and the few hundred additions of a block are exact in fp32, so the partial sums equal the fp64 ones
(dbeta 0.000 on every case).  rpa likewise on gauss data (0.19 with posg).

Injected defects (test_injected_defect_lands_outside_the_bound, test_stem_injected_defect_...), each outside the bound
on its named case, and how many cases of the old tests they pass (test_old_tolerances_on_record: the emulation with the
defect through the assert_close tolerances of tests/test_gpu_bn.py::test_bn_act_forward_backward, 18 cases, and of
test_stem_bn_relu_pool_matches_unfused, 4 shapes, on those tests' shapes and data):

    defect                                                  outside on              old tests passed
    no_k2         dx without the -k2 term                   531x64 posg   cD, dxt    6 of 18
    bf16_mean     B, D from a mean rounded to bf16          531x64 off300 cD, dxt   15 of 18
    var_noshift   fp32 E[x^2] - E[x]^2 without the shift    531x64 off300 invstd    18 of 18
    rvar_biased   running variance without M / (M - 1)      531x64        rvar       6 of 18
    l1_neighbour  level-1 partial to the next block row     531x64        l1*       18 of 18 (the totals are unchanged)
    drop_tail     the last M % R rows dropped               513x64        mean, ..   9 of 18
    rp_half       half of each ResBn row unwritten (G=512)  300x4096      rpa, rpb   not reachable on those shapes
    pool_last     last maximum instead of the first         2x8x16x15 equal pixels   1 of 4
    mask_ypool    stem backward masked by y_pooled > 0      1x64x17x16 random idx    4 of 4

rp_half is what bn_bwd_dx_kernel<RP = true> did at C = 4096 before plx_bn_backward refused a ResBn above 256 channel
groups: a block covers 256 of the 512 groups of its row of `part`, the combine loop `j < 256 / G` runs zero times, and
the other half of the row stays as allocated.  _BNAct no longer arms the residual link above C = 2048 (the residual
BatchNorm runs its own reduce; test_gpu_autograd_residual_link[4096]).  mask_ypool equals the kernel's rule whenever
the positions are the forward's own (a pixel that is a window's maximum has y_pooled = its own f); it shows only with
positions the test hands over.

Bound terms that rest on a reading of the code, not on a measurement: rsqrtf within 2 ulp (measured 0.18 of the invstd
bound at most), a correctly rounded or 2.5-ulp fp32 division for k2 / k3, and hipcc's freedom to contract
`a * b + c` into an fma in the finalize (the bounds charge the unfused roundings, which cover both).
"""
import math
import zlib
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -8            # bf16 round-to-nearest unit roundoff
E = 2.0 ** -24           # fp32 unit roundoff
RSQ = 4 * E              # rsqrtf: 2 ulp
L2_CHAIN = 20            # l1_rows<1024> (:134: 4 rows per thread) + the 16-group combine (:153 / :303)
EPS, MOM = 1e-5, 0.1
GUARD = {torch.bfloat16: (torch.int16, 0x7B7B), torch.float32: (torch.int32, 0x7B7B7B7B),
         torch.uint8: (torch.uint8, 0x7B)}
_F32, _F64, _BF = torch.float32, torch.float64, torch.bfloat16


def _gamma(k):
    return k * E / (1 - k * E)


def _f32(v) -> float:
    """The kernels take eps and momentum as float arguments."""
    return float(torch.tensor(v, dtype=_F32))


# ------------------------------------------------------------------------------ the launch geometry of bn_kernels.hip
Plan = namedtuple("Plan", "G Gb gy R rpb nblk S")


def _plan(M, C) -> Plan:
    """plan_for (:610)."""
    G = C // 8
    assert M >= 1 and C % 8 == 0 and G & (G - 1) == 0
    Gb = min(G, 256)
    gy, R = G // Gb, 256 // Gb
    want = max(1, min(-(-M // (16 * R)), -(-2048 // gy)))
    rpb = -(-(-(-M // want)) // R) * R
    nblk = -(-M // rpb)
    return Plan(G, Gb, gy, R, rpb, nblk, -(-nblk // 64))


def _apply_grid(n_vec, G) -> int:
    """apply_grid (:631)."""
    g = max(1, min(-(-n_vec // 256), 4096))
    mult = G // 256 if G > 256 else 1
    return -(-g // mult) * mult


def _l1_chain(p: Plan) -> int:
    """Additions a level-1 partial passes through: a thread's rows_per_block / R rows (:79, :451), then the R - 1
    adds of the LDS combine (:96, :475)."""
    return p.rpb // p.R + p.R - 1


def _rp_chain(M, G) -> int:
    """ResBn partials: a thread's trips of the grid-stride loop (:549), then the 256 / G - 1 adds of the LDS combine
    (:586)."""
    nv = M * G
    return -(-nv // (_apply_grid(nv, G) * 256)) + max(256 // G, 1) - 1


# ------------------------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "m c kind relu res ext cnt rb opt")


def _mk(m, c, kind="gauss", relu=True, res=0, ext=0, cnt=True, rb=0, opt="") -> Case:
    """res: 0 none, 1 residual, 2 residual with res_sb; ext: rows of external partials (0: own pass); cnt: one-launch
    reduce + finalize; rb: 0 none, 1 ResBn, 2 ResBn with its mask; opt: 'coef' (dx = None), 'acc', 'ynone'."""
    return Case(m, c, kind, relu, res, ext, cnt, rb, opt)


def _id(c: Case) -> str:
    return (f"{c.m}x{c.c}-{c.kind}" + ("-relu" if c.relu else "") + ("", "-res", "-ressb")[c.res]
            + (f"-ext{c.ext}" if c.ext else "") + ("" if c.cnt else "-2launch") + ("", "-rb", "-rbmask")[c.rb]
            + (f"-{c.opt}" if c.opt else ""))


def _layout_cases():
    out = []
    variants = [dict(relu=True, res=1), dict(relu=False), dict(relu=True, res=2, rb=1), dict(relu=True, cnt=False),
                dict(relu=False, res=1, rb=2), dict(relu=True, opt="acc")]
    for C in (8, 16, 64, 2048, 4096):
        R = _plan(1, C).R
        for i, M in enumerate(sorted({m for m in (1, 2, R - 1, R, R + 1, 16 * R + 1) if m >= 1})):
            v = dict(variants[(i + C // 8) % len(variants)])
            if C > 2048:
                v.pop("rb", None)  # plx_bn_backward refuses a ResBn above 256 channel groups
            out.append(_mk(M, C, **v))
    return out


LAYOUT = _layout_cases()
# nblk on both sides of one level-2 split (64 rows), and C = 4096 at the 2048 / gy cap of plan_for
SPLIT = [_mk(1024, 2048), _mk(1040, 2048, res=1), _mk(16400, 4096, relu=False)]
# n_vec > 4096 * 256: the grid-stride loop of apply / dx takes a second trip.  (apply_grid's rounding to a multiple of
# G / 256 never changes the grid: n_vec = M * G is a multiple of G, so ceil(n_vec / 256) already is one of G / 256)
GRID = [_mk(16400, 512, res=1, rb=2)]
# S = ceil(ext / 64) across 1 -> 2 and 128 -> 129 (the second trip of fin_sum2); the GPU test runs each case with and
# without counters
EXT = [_mk(2 * e + 3, 64, ext=e, res=1) for e in (1, 63, 64, 65, 8192, 8193, 8257)]
VARIANTS = ([_mk(100, 64, relu=r, res=s) for r in (False, True) for s in (0, 1, 2)]
            + [_mk(100, 64, relu=r, res=s, rb=b) for r in (False, True) for s in (0, 1) for b in (1, 2)]
            + [_mk(100, 64, relu=o != "ynone", opt=o, res=s) for o in ("coef", "acc", "ynone") for s in (0, 1)
               if not (o == "coef" and s)]
            + [_mk(300, 2048, rb=1), _mk(300, 4096, res=1)])
_KINDS = ("gauss", "off300", "row0out", "const", "posg", "widegamma")
KINDS = [_mk(m, c, k, res=1, rb=2) for k in _KINDS for m, c in ((531, 64), (45, 256))]
KINDS += [_mk(2 * 130 + 3, 64, k, ext=130) for k in ("gauss", "off300", "posg")]
CASES = list(dict.fromkeys(LAYOUT + SPLIT + GRID + EXT + VARIANTS + KINDS))
CPU_CASES = [c for c in CASES if c.m * c.c <= 1 << 21]

Inputs = namedtuple("Inputs", "x res rsb gamma beta rm0 rv0 dy x2 mask2 mean2 is2 dg0 db0 fpart")


def _blk_of_row(M, nblk, dev):
    return (torch.arange(M, device=dev) * nblk) // M


def _ext_sums(a, b, nblk):
    """fp32 [2][nblk][C] partial sums of the fp64 [M, C] terms a and b over nblk consecutive row blocks: what a
    producing GEMM's epilogue hands over."""
    M, C = a.shape
    key = _blk_of_row(M, nblk, a.device)
    z = lambda v: torch.zeros(nblk, C, dtype=_F64, device=a.device).index_add_(0, key, v)  # noqa: E731
    return torch.stack([z(a), z(b)]).float()


def _inputs(c: Case) -> Inputs:
    """The tensors of a case (CPU): bf16 x, res, dy, x2 [M, C]; fp32 per-channel vectors."""
    # one data set for both launch paths
    gen = torch.Generator().manual_seed(zlib.crc32(_id(c._replace(cnt=True)).encode()))
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    M, C = c.m, c.c
    x, dy, res = 2.0 * rnd(M, C) + 0.5, rnd(M, C), rnd(M, C)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, 0.1 * rnd(C)
    if c.kind == "off300":       # bf16 spacing 2 at 300; dy follows x, so dgamma / M (k3) is of order 1
        x = rnd(M, C) + 300.0
        dy = dy + 0.5 * (x.bfloat16().float() - 300.0)
    elif c.kind == "row0out":
        x = rnd(M, C)
        x[0] += 50.0
    elif c.kind == "const":
        x = (0.25 * (torch.arange(C) % 16) - 2.0).expand(M, C).clone()
    elif c.kind == "posg":
        dy = dy.abs()
    elif c.kind == "widegamma":
        gamma = rnd(C) * torch.exp2(torch.randint(-6, 7, (C,), generator=gen).float())
        gamma[::5] = 0.0
    bf = lambda t: t.to(_BF)  # noqa: E731
    x = bf(x)
    G = C // 8
    rsb = torch.cat([torch.rand(C, generator=gen) + 0.5, 0.3 * rnd(C)]) if c.res == 2 else None
    fpart = _ext_sums(x.double(), x.double() ** 2, c.ext) if c.ext else None
    return Inputs(x, bf(res) if c.res else None, rsb, gamma, beta, 0.1 * rnd(C), torch.rand(C, generator=gen) + 0.5,
                  bf(dy), bf(rnd(M, C)),
                  torch.randint(0, 256, (M * G,), generator=gen, dtype=torch.int32).to(torch.uint8), 0.2 * rnd(C),
                  torch.rand(C, generator=gen) + 0.5, rnd(C), rnd(C), fpart)


def _on(inp: Inputs, dev) -> Inputs:
    return Inputs(*(None if t is None else t.to(dev) for t in inp))


def _unpack(mask, M, C):
    """[M * C / 8] mask bytes -> bool [M, C] (bit k of byte i = channel 8 * (i % G) + k of row i / G, :417)."""
    k = torch.arange(8, device=mask.device, dtype=torch.int32)
    return ((mask.to(torch.int32).view(-1, 1) >> k) & 1).bool().view(M, C)


def _pack(bits):
    k = torch.arange(8, device=bits.device, dtype=torch.int32)
    return (bits.view(-1, 8).to(torch.int32) << k).sum(1).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------ the oracle
def _rowblocks(V, p: Plan):
    """fp64 sums of V [M, C] over the row blocks of the own statistics / reduce pass (:75, :447)."""
    M, C = V.shape
    pad = p.nblk * p.rpb - M
    if pad:
        V = torch.cat([V, V.new_zeros(pad, C)])
    return V.view(p.nblk, p.rpb, C).sum(1)


def _sums(a, b, k_a, k_b, p, part, blocks=None):
    """Level-1 references / bounds of the two sums (None with external partials), the fp64 totals and their bounds.
    Own pass: the terms a, b [M, C] in fp64 with k_a, k_b roundings per term on top of the chain; external: the
    given fp32 partials are inputs, only level 2 is charged.  fin_sum2 (:165) adds in fp64 and is charged nothing.
    ``blocks``: (block sums of a [M, C] tensor, chain) of another level-1 pass (the stem's) in the plan's place."""
    if part is not None:
        P = part.double()
        return None, (P[0].sum(0), P[1].sum(0)), (_gamma(L2_CHAIN) * P[0].abs().sum(0),
                                                  _gamma(L2_CHAIN) * P[1].abs().sum(0))
    bs, k = blocks if blocks is not None else (lambda V: _rowblocks(V, p), _l1_chain(p))
    ra, rb, aa, ab = bs(a), bs(b), bs(a.abs()), bs(b.abs())
    l1 = ((ra, _gamma(k + k_a) * aa), (rb, _gamma(k + k_b) * ab))
    return l1, (ra.sum(0), rb.sum(0)), (_gamma(k + k_a + L2_CHAIN) * aa.sum(0), _gamma(k + k_b + L2_CHAIN) * ab.sum(0))


def _oracle_fwd(x, gamma, beta, rm0, rv0, eps, mom, part=None):
    """Statistics of x [M, C]: (ref, bound) dicts of mean, invstd, scale, bias, rmean, rvar, and l1 (own pass)."""
    M, C = x.shape
    p = _plan(M, C)
    X, g, bt = x.double(), gamma.double(), beta.double()
    eps, mom = _f32(eps), _f32(mom)
    # own pass: d = fl(x - x[0]) (:84, one rounding), s += d, q = fmaf(d, d, q) (:85-86: d's rounding twice, the fma's)
    shift = X[0] if part is None else torch.zeros(C, dtype=_F64, device=x.device)
    D = X - shift
    l1, (S, Q), (dS, dQ) = _sums(D, D * D, 1, 3, p, part)
    # m = S / M, var = Q / M - m^2 in fp64 (:236-237) on the fp32 sums; the clamp at 0 (:238) only shrinks an error
    m = S / M
    var = (Q / M - m * m).clamp_min(0)
    dvar = dQ / M + 2 * m.abs() * dS / M + (dS / M) ** 2 + 2.0 ** -50 * (Q / M + m * m)
    # mean = shift + (float)m (:239)
    mean = shift + m
    b_m = dS / M + E * m.abs()
    b_mean = b_m + E * (mean.abs() + b_m)
    # invstd = rsqrtf((float)var + eps) (:240): the cast and the add relative to var + eps, rsqrtf at half weight
    ve = var + eps
    e_v = (dvar + E * var) / ve + 2 * E
    e_is = 0.5 * e_v / (1 - e_v.clamp(max=0.5)) + RSQ
    invstd = ve.rsqrt()
    b_is = invstd * e_is
    # scale = g * invstd (:244); bias = beta - mean * g * invstd (:245): the product's error is absolute, so a beta
    # that cancels it does not shrink it
    scale = g * invstd
    b_scale = g.abs() * b_is + E * (scale.abs() + g.abs() * b_is)
    P = mean * g * invstd
    b_P = g.abs() * (mean.abs() * b_is + invstd * b_mean + b_is * b_mean) + 3 * E * P.abs()
    bias = bt - P
    b_bias = b_P + E * (bias.abs() + b_P)
    # running statistics (:247-249): unbiased = (float)(var * M / (M - 1)), r = (1 - mom) * r + mom * stat
    a = 1.0 - mom
    unb = var * M / (M - 1) if M > 1 else var
    b_unb = (dvar * M / (M - 1) if M > 1 else dvar) + E * unb
    rmean = a * rm0.double() + mom * mean
    b_rmean = mom * b_mean + 3 * E * ((a * rm0.double()).abs() + (mom * mean).abs())
    rvar = a * rv0.double() + mom * unb
    b_rvar = mom * b_unb + 3 * E * ((a * rv0.double()).abs() + mom * unb)
    ref = dict(mean=mean, invstd=invstd, scale=scale, bias=bias, rmean=rmean, rvar=rvar)
    bound = dict(mean=b_mean, invstd=b_is, scale=b_scale, bias=b_bias, rmean=b_rmean, rvar=b_rvar)
    if l1 is not None:
        ref.update(l1s=l1[0][0], l1q=l1[1][0])
        bound.update(l1s=l1[0][1], l1q=l1[1][1])
    return ref, bound


def _oracle_apply(x, scale, bias, res=None, rsb=None, relu=False):
    """y = bf16(act(fmaf(x, a, b) [+ fmaf(res, ra, rb)])) (:406-415) from the fp32 scale / bias given: each fma and the
    add round once in fp32, the store once to bf16; ReLU is 1-Lipschitz, so no element is special."""
    C = x.shape[1]
    t = x.double() * scale.double() + bias.double()
    err = E * t.abs()
    Z = t
    if res is not None:
        r = res.double()
        if rsb is not None:
            r = r * rsb[:C].double() + rsb[C:].double()
            err = err + E * r.abs()
        Z = t + r
        err = err + E * (Z.abs() + err)
    Y = Z.clamp_min(0) if relu else Z
    return Y, U * Y.abs() + (1 + U) * err


def _oracle_bwd(x, dz, gamma, mean, invstd, part=None, acc=None, blocks=None):
    """The reduce and the finalize from the fp32 mean / invstd given and dz [M, C] (dy under the mask given): (ref,
    bound) of l1a, l1b (own pass), dbeta, dgamma, the coefficients cA, cB, cD, and the per-element coefficient error
    of the textbook dx = k1 * (dz - k2 - xhat * k3)."""
    M, C = x.shape
    p = _plan(M, C)
    X, DZ, g, mu, is_ = x.double(), dz.double(), gamma.double(), mean.double(), invstd.double()
    # sa += dz, sb = fmaf(dz, fl(fl(x - mu) * is), sb) (:464-465): two roundings of xhat and the fma's
    XH = (X - mu) * is_
    l1, (A, B), (dA, dB) = _sums(DZ, DZ * XH, 0, 3, p, part, blocks)
    b_db, b_dg = dA + E * A.abs(), dB + E * B.abs()          # db = (float)A, dg = (float)B (:259)
    ref, bound = dict(dbeta=A, dgamma=B), dict(dbeta=b_db, dgamma=b_dg)
    if acc is not None:                                       # dbeta[c] + db (:261-262)
        dg0, db0 = acc
        ref.update(dbeta=A + db0.double(), dgamma=B + dg0.double())
        bound.update(dbeta=b_db + E * (ref["dbeta"].abs() + b_db), dgamma=b_dg + E * (ref["dgamma"].abs() + b_dg))
    # k1 = g * is, k2 = db / M, k3 = dg / M (:263-264; the division is charged 2.5 ulp)
    k1, k2, k3 = g * is_, A / M, B / M
    b_k2, b_k3 = b_db / M + 3 * E * k2.abs(), b_dg / M + 3 * E * k3.abs()
    cB = -k1 * k3 * is_                                       # (:267) k1's rounding and two products
    b_cB = (k1 * is_).abs() * b_k3 + 4 * E * cB.abs()
    T1, T2 = k1 * k2, k1 * k3 * is_ * mu                      # (:268) D = -T1 + T2: the terms cancel when the mean is
    cD = -T1 + T2                                             # large, so each is charged at its own size
    b_cD = k1.abs() * b_k2 + (k1 * is_ * mu).abs() * b_k3 + 6 * E * (T1.abs() + T2.abs())
    ref.update(cA=k1, cB=cB, cD=cD, dxt=k1 * (DZ - k2 - XH * k3))
    bound.update(cA=E * k1.abs(), cB=b_cB, cD=b_cD, dxt=DZ.abs() * E * k1.abs() + X.abs() * b_cB + b_cD)
    if l1 is not None:
        ref.update(l1a=l1[0][0], l1b=l1[1][0])
        bound.update(l1a=l1[0][1], l1b=l1[1][1])
    return ref, bound


def _oracle_dx(x, dz, coef):
    """dx = bf16(fmaf(A, dz, fmaf(B, x, D))) (:573) from the fp32 coefficients given [3, C]."""
    A, B, D = (coef[i].double() for i in range(3))
    t = B * x.double() + D
    DX = A * dz.double() + t
    return DX, U * DX.abs() + (1 + U) * (E * t.abs() + E * (DX.abs() + E * t.abs()))


def _oracle_resbn(x2, dz, bits2, mean2, is2):
    """ResBn partials [2][grid][C] (:560-600): block b of the dx pass sums the vectors i = b * 256 + t + j * stride."""
    M, C = x2.shape
    G = C // 8
    grid = _apply_grid(M * G, G)
    i = torch.arange(M * G, device=x2.device)
    key = ((i % (grid * 256)) // 256) * G + i % G
    DZ = dz.double() * bits2 if bits2 is not None else dz.double()
    T = DZ * ((x2.double() - mean2.double()) * is2.double())
    z = lambda v: torch.zeros(grid * G, 8, dtype=_F64, device=x2.device).index_add_(  # noqa: E731
        0, key, v.reshape(M * G, 8)).view(grid, C)
    k = _rp_chain(M, G)
    return dict(rpa=z(DZ), rpb=z(T)), dict(rpa=_gamma(k) * z(DZ.abs()), rpb=_gamma(k + 3) * z(T.abs()))


def _ratio(got, ref, bound) -> float:
    """max |got - ref| / bound.  A bound of exactly 0 means the element must be exact; NaN must sit exactly where
    the reference has it."""
    got = got.double().reshape(ref.shape)
    bound = bound.expand_as(ref)
    nan = ref.isnan()
    if not torch.equal(got.isnan(), nan):
        return math.inf
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(nan, torch.zeros_like(r), r).nan_to_num(nan=math.inf, posinf=math.inf)
    return float(r.max()) if r.numel() else 0.0


def _fmt(r: dict) -> str:
    return " ".join(f"{n}={x:.3f}" for n, x in r.items())


def _check(c: Case, inp: Inputs, fo: dict, bo: dict, keep=None) -> dict:
    """Ratios of every output of a forward (fo) and backward (bo) call of a case.  ``keep``: bool [C], the channels
    to judge (NaN containment)."""
    M, C = c.m, c.c
    sel = (lambda t: t) if keep is None else (lambda t: t[..., keep])  # noqa: E731
    r = {}
    ref, bound = _oracle_fwd(inp.x, inp.gamma, inp.beta, inp.rm0, inp.rv0, EPS, MOM, inp.fpart)
    for n in ref:
        r[n] = _ratio(sel(fo[n]), sel(ref[n]), sel(bound[n]))
    if fo["y"] is not None:
        # from the scale / bias the kernel stored (held to their own bounds above)
        Y, b_y = _oracle_apply(inp.x, fo["scale"], fo["bias"], inp.res, inp.rsb, c.relu)
        r["y"] = _ratio(sel(fo["y"]), sel(Y), sel(b_y))
        if c.relu:  # the bit equals y > 0 of the y the kernel stored (:417)
            r["mask"] = 0.0 if torch.equal(sel(_unpack(fo["mask"], M, C)), sel(fo["y"].float() > 0)) else math.inf
    if bo is None:
        return r
    bits = bo["bits"]
    dz = inp.dy.float() * bits if bits is not None else inp.dy.float()
    ref, bound = _oracle_bwd(inp.x, dz, inp.gamma, fo["mean"], fo["invstd"], bo["ext"],
                             (inp.dg0, inp.db0) if c.opt == "acc" else None)
    for n in ("l1a", "l1b", "dbeta", "dgamma"):
        if n in ref:
            r[n] = _ratio(sel(bo[n]), sel(ref[n]), sel(bound[n]))
    for i, n in enumerate(("cA", "cB", "cD")):
        r[n] = _ratio(sel(bo["coef"][i]), sel(ref[n]), sel(bound[n]))
    if bo["dx"] is not None:
        DX, b_dx = _oracle_dx(inp.x, dz, bo["coef"])
        r["dx"] = _ratio(sel(bo["dx"]), sel(DX), sel(b_dx))
        r["dxt"] = _ratio(sel(bo["dx"]), sel(ref["dxt"]), sel(b_dx + bound["dxt"]))
    if bo["dres"] is not None:  # dz stored to bf16 from bf16: bit-exact
        r["dres"] = 0.0 if torch.equal(sel(bo["dres"]), sel(dz.to(_BF))) else math.inf
    if bo["rpart"] is not None:
        bits2 = _unpack(inp.mask2, M, C) if c.rb == 2 else None
        ref, bound = _oracle_resbn(inp.x2, dz, bits2, inp.mean2, inp.is2)
        for i, n in enumerate(("rpa", "rpb")):
            r[n] = _ratio(sel(bo["rpart"][i]), sel(ref[n]), sel(bound[n]))
    return r


# ----------------------------------------------------------------------------- fp32 emulation of the kernels (CPU)
def _fma(a, b, c):
    """fmaf on fp32 tensors, exactly: a * b is exact in fp64 (24 + 24 bits); TwoSum gives the fp64 sum s and its exact
    error; where s is inexact and lies midway between two fp32 numbers, the error's sign decides instead of a second
    round-to-even."""
    a, b, c = torch.broadcast_tensors(a, b, c)
    p, cd = a.double() * b.double(), c.double()
    s = p + cd
    bv = s - p
    err = (p - (s - bv)) + (cd - bv)
    r = s.float()
    d = s - r.double()
    r2 = torch.nextafter(r, torch.where(d > 0, math.inf, -math.inf).to(_F32))
    tie = (d != 0) & (err != 0) & (d == r2.double() - s)
    return torch.where(tie & ((err > 0) == (d > 0)), r2, r)


def _emu_l1(p: Plan, t, fa, fb, defect=None):
    """bn_stats_kernel / bn_bwd_reduce_kernel: s += t, q = fmaf(fa, fb, q) over the rows r0 + rlane, + R, ... of a
    block in order, then lane 0 adds the R lanes in order.  -> fp32 [2, nblk, C]."""
    M, C = t.shape
    R, n_t = p.R, p.rpb // p.R
    if defect == "drop_tail" and M % R:
        keep = torch.arange(M) < M - M % R
        t, fa = t * keep[:, None], fa * keep[:, None]
    pad = p.nblk * p.rpb - M
    z = lambda v: torch.cat([v, v.new_zeros(pad, C)]).view(p.nblk, n_t, R, C)  # noqa: E731
    t, fa, fb = z(t), z(fa), z(fb)
    s = torch.zeros(p.nblk, R, C)
    q = torch.zeros(p.nblk, R, C)
    for j in range(n_t):
        s = s + t[:, j]
        q = _fma(fa[:, j], fb[:, j], q)
    S, Q = s[:, 0], q[:, 0]
    for j in range(1, R):
        S, Q = S + s[:, j], Q + q[:, j]
    out = torch.stack([S, Q])
    if defect == "l1_neighbour":
        out = out.roll(1, dims=1)
    return out


def _emu_l2(part):
    """l1_rows<1024> (:124) + the group combine (:153): per split of 64 rows, lane l adds rows l, l + 16, l + 32,
    l + 48 in order, then the 16 lanes are added in order.  [nblk, C] -> [S, C]."""
    nblk, C = part.shape
    S = -(-nblk // 64)
    v = torch.cat([part, part.new_zeros(S * 64 - nblk, C)]).view(S, 4, 16, C)
    a = torch.zeros(S, 16, C)
    for u in range(4):
        a = a + v[:, u]
    r = torch.zeros(S, C)
    for g in range(16):
        r = r + a[:, g]
    return r


def _emu_fin(l2):
    """fin_sum2<1024> (:165): group sp adds the rows sp, sp + 16, ... in fp64, then the 16 groups in order."""
    d = l2.double()
    tot = torch.zeros(d.shape[1], dtype=_F64)
    for sp in range(16):
        a = torch.zeros(d.shape[1], dtype=_F64)
        for b in range(sp, d.shape[0], 16):
            a = a + d[b]
        tot = tot + a
    return tot


def _emu_forward(c: Case, inp: Inputs, defect=None) -> dict:
    M, C = c.m, c.c
    p = _plan(M, C)
    xf = inp.x.float()
    eps, mom = torch.tensor(EPS, dtype=_F32), torch.tensor(MOM, dtype=_F32)
    if c.ext:
        shift, part, l1 = torch.zeros(C), inp.fpart, None
    else:
        shift = torch.zeros(C) if defect == "var_noshift" else xf[0]
        d = xf - shift
        part = l1 = _emu_l1(p, d, d, d, defect)
    S, Q = _emu_fin(_emu_l2(part[0])), _emu_fin(_emu_l2(part[1]))
    m = S / M
    var = (Q / M - m * m).clamp_min(0)
    if defect == "var_noshift":  # plain fp32 E[x^2] - E[x]^2
        m32 = S.float() / M
        var = (Q.float() / M - m32 * m32).clamp_min(0).double()
    mean = shift + m.float()
    invstd = (var.float() + eps).double().rsqrt().float()
    g = inp.gamma
    scale = g * invstd
    bias = inp.beta - mean * g * invstd
    unb = var if (M == 1 or defect == "rvar_biased") else var * M / (M - 1)
    rmean = (1 - mom) * inp.rm0 + mom * mean
    rvar = (1 - mom) * inp.rv0 + mom * unb.float()
    out = dict(mean=mean, invstd=invstd, scale=scale, bias=bias, rmean=rmean, rvar=rvar, y=None, mask=None)
    if l1 is not None:
        out.update(l1s=l1[0], l1q=l1[1])
    if c.opt != "ynone":
        v = _fma(xf, scale, bias)
        if inp.res is not None:
            r = inp.res.float()
            if inp.rsb is not None:
                r = _fma(r, inp.rsb[:C], inp.rsb[C:])
            v = v + r
        if c.relu:
            v = v.clamp_min(0)
            out["mask"] = _pack(v > 0)
        out["y"] = v.to(_BF)
    return out


def _emu_resbn(inp: Inputs, dz, M, C, rb, defect=None):
    """The ResBn partials of bn_bwd_dx_kernel<RP = true> (:560-600), fp32 [2, grid, C]."""
    G = C // 8
    nv = M * G
    grid = _apply_grid(nv, G)
    stride = grid * 256
    trips = -(-nv // stride)
    g2 = dz * _unpack(inp.mask2, M, C) if rb == 2 else dz
    xh2 = (inp.x2.float() - inp.mean2) * inp.is2
    pad = trips * stride - nv
    z = lambda v: torch.cat([v.reshape(nv, 8), v.new_zeros(pad, 8)]).view(trips, grid, 256, 8)  # noqa: E731
    g2, xh2 = z(g2), z(xh2)
    ra, rc = torch.zeros(grid, 256, 8), torch.zeros(grid, 256, 8)
    for t in range(trips):
        ra = ra + g2[t]
        rc = _fma(g2[t], xh2[t], rc)
    if G > 256:
        # the kernel before its entry point refused G > 256: `threadIdx.x < G` holds for all 256 threads, the combine
        # loop `j < 256 / G` runs zero times, and block b writes only the 256 groups (b * 256 + t) % G of its row
        assert defect == "rp_half"
        out = torch.full((2, grid, G, 8), math.nan)
        for b in range(grid):
            o = (b * 256) % G
            out[0, b, o:o + 256], out[1, b, o:o + 256] = ra[b], rc[b]
        return out.view(2, grid, C)
    va, vc = ra.view(grid, 256 // G, G, 8), rc.view(grid, 256 // G, G, 8)
    A, B = va[:, 0], vc[:, 0]
    for j in range(1, 256 // G):
        A, B = A + va[:, j], B + vc[:, j]
    return torch.stack([A, B]).reshape(2, grid, C)


def _emu_backward(c: Case, inp: Inputs, fo: dict, ext, defect=None) -> dict:
    M, C = c.m, c.c
    p = _plan(M, C)
    xf = inp.x.float()
    bits = _unpack(fo["mask"], M, C) if c.relu else None
    dz = inp.dy.float() * bits if c.relu else inp.dy.float()
    mean, is_, g = fo["mean"], fo["invstd"], inp.gamma
    out = dict(bits=bits, ext=ext, dx=None, dres=None, rpart=None)
    if ext is None:
        l1 = _emu_l1(p, dz, dz, (xf - mean) * is_, defect)
        out.update(l1a=l1[0], l1b=l1[1])
    else:
        l1 = ext
    db, dg = _emu_fin(_emu_l2(l1[0])).float(), _emu_fin(_emu_l2(l1[1])).float()
    acc = c.opt == "acc"
    out.update(dbeta=inp.db0 + db if acc else db, dgamma=inp.dg0 + dg if acc else dg)
    k1 = g * is_
    k2, k3 = db / float(M), dg / float(M)
    mu = mean.to(_BF).float() if defect == "bf16_mean" else mean
    cD = k1 * k3 * is_ * mu if defect == "no_k2" else -k1 * k2 + k1 * k3 * is_ * mu
    out["coef"] = torch.stack([k1, -k1 * k3 * is_, cD])
    if c.opt != "coef":
        out["dx"] = _fma(k1, dz, _fma(out["coef"][1], xf, cD)).to(_BF)
        if c.res or c.rb:
            out["dres"] = dz.to(_BF)
        if c.rb:
            out["rpart"] = _emu_resbn(inp, dz, M, C, c.rb, defect)
    return out


def _bwd_ext(c: Case, inp: Inputs, fo: dict):
    """External partials of the backward, generated by the test: fp32 block sums of dz and dz * xhat."""
    if not c.ext:
        return None
    dz = inp.dy.double() * (_unpack(fo["mask"], c.m, c.c) if c.relu else 1.0)
    xh = (inp.x.double() - fo["mean"].double()) * fo["invstd"].double()
    return _ext_sums(dz, dz * xh, c.ext)


def _emu_run(c: Case, defect=None, inp=None):
    inp = _inputs(c) if inp is None else inp
    fo = _emu_forward(c, inp, defect)
    if c.opt == "ynone" and c.relu:
        return _check(c, inp, fo, None), fo, None
    bo = _emu_backward(c, inp, fo, _bwd_ext(c, inp, fo), defect)
    return _check(c, inp, fo, bo), fo, bo


def _family(c: Case) -> str:
    return "ext" if c.ext else "own"


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_plan_matches_the_documented_layout():
    """The geometry helpers give the issue's figures: Gb and gy per channel count, the level-2 split at nblk = 64,
    the cap at C = 4096, the second grid-stride trip."""
    assert [(_plan(1, C).Gb, _plan(1, C).gy) for C in (8, 16, 64, 2048, 4096)] == [(1, 1), (2, 1), (8, 1), (256, 1),
                                                                                   (256, 2)]
    assert (_plan(1024, 2048).nblk, _plan(1024, 2048).S) == (64, 1)
    assert (_plan(1040, 2048).nblk, _plan(1040, 2048).S) == (65, 2)
    assert _plan(16400, 4096).rpb == 17 and _plan(16400, 4096).nblk == 965
    assert 16400 * 64 > 4096 * 256 and _apply_grid(16400 * 64, 64) == 4096
    assert all(_apply_grid(m * 512, 512) == min(2 * m, 4096) for m in (1, 3, 2047, 2049, 5000))


def test_oracle_matches_torch_batch_norm():
    """The oracle's statistics, y and textbook dx equal torch's fp64 batch_norm and its autograd."""
    torch.manual_seed(0)
    M, C = 37, 16
    x = torch.randn(M, C).to(_BF)
    dy = torch.randn(M, C).to(_BF)
    g, b = torch.rand(C) + 0.5, torch.randn(C)
    rm, rv = torch.randn(C), torch.rand(C) + 0.5
    ref, _ = _oracle_fwd(x, g, b, rm, rv, EPS, MOM)
    xr = x.double().requires_grad_()
    gr, br = g.double().requires_grad_(), b.double().requires_grad_()
    rm2, rv2 = rm.double().clone(), rv.double().clone()
    yr = F.relu(F.batch_norm(xr, rm2, rv2, gr, br, True, _f32(MOM), _f32(EPS)))
    Y, _ = _oracle_apply(x, ref["scale"], ref["bias"], relu=True)
    assert torch.allclose(Y, yr, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["rmean"], rm2, rtol=1e-12) and torch.allclose(ref["rvar"], rv2, rtol=1e-12)
    yr.backward(dy.double())
    dz = dy.double() * (yr > 0)
    rb, _ = _oracle_bwd(x, dz, g, ref["mean"], ref["invstd"])
    assert torch.allclose(rb["dxt"], xr.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(rb["dgamma"], gr.grad, rtol=1e-10) and torch.allclose(rb["dbeta"], br.grad, rtol=1e-10)
    coef = torch.stack([rb["cA"], rb["cB"], rb["cD"]])
    assert torch.allclose(_oracle_dx(x, dz, coef)[0], xr.grad, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("case", CPU_CASES, ids=_id)
def test_emulation_stays_inside_the_bound(case):
    r, _, _ = _emu_run(case)
    print(f"BN_RATIO emu {_family(case)} {_id(case)}: {_fmt(r)}")
    assert max(r.values()) <= 1.0, _fmt(r)


# defect -> (the case that must catch it, the quantities that land outside the bound there)
DEFECTS = {
    "no_k2": (_mk(531, 64, "posg", res=1, rb=2), ("cD", "dxt")),
    "bf16_mean": (_mk(531, 64, "off300", res=1, rb=2), ("cD", "dxt")),
    "var_noshift": (_mk(531, 64, "off300", res=1, rb=2), ("invstd",)),
    "rvar_biased": (_mk(531, 64, "gauss", res=1, rb=2), ("rvar",)),
    "l1_neighbour": (_mk(531, 64, "gauss", res=1, rb=2), ("l1s", "l1q", "l1a", "l1b")),
    "drop_tail": (_mk(16 * 32 + 1, 64, relu=True, opt="acc"), ("mean", "dbeta")),
    "rp_half": (_mk(300, 4096, res=1, rb=1), ("rpa", "rpb")),
}


@pytest.mark.parametrize("defect", list(DEFECTS), ids=str)
def test_injected_defect_lands_outside_the_bound(defect):
    case, quantities = DEFECTS[defect]
    r, _, _ = _emu_run(case, defect)
    print(f"BN_RATIO defect {defect} {_id(case)}: {_fmt(r)}")
    for q in quantities:
        assert r[q] > 1.0, (q, _fmt(r))
    if defect != "rp_half":  # the same case is clean without the defect (C = 4096 with a ResBn is now refused)
        assert max(_emu_run(case)[0].values()) <= 1.0


# tests/test_gpu_bn.py::test_bn_act_forward_backward: its shapes, data and tolerances
_OLD_SHAPES = [(4, 64, 14, 14), (2, 256, 7, 9), (3, 2048, 3, 3), (2, 4096, 2, 2), (2, 128, 1, 1), (8, 64, 56, 56)]
_OLD_VARIANTS = [(True, False), (True, True), (False, False)]
# measured by test_old_tolerances_on_record: how many of the old test's 18 cases pass with the defect in place
OLD_ACCEPTS = {"no_k2": 6, "bf16_mean": 15, "var_noshift": 18, "rvar_biased": 6, "l1_neighbour": 18, "drop_tail": 9}
# ... and of the 4 shapes of test_stem_bn_relu_pool_matches_unfused (the clean emulation in the unfused path's place)
OLD_STEM_SHAPES = [(4, 64, 112, 112), (3, 64, 15, 17), (2, 128, 9, 8), (2, 8, 6, 5)]
OLD_STEM_ACCEPTS = {"pool_last": 1, "mask_ypool": 4}


def _old_test_passes(defect, shape, relu, residual) -> bool:
    n, ch, h, w = shape
    M = n * h * w
    torch.manual_seed(0)
    x = (torch.randn(M, ch) * 2 + 0.5).to(_BF)
    res = torch.randn(M, ch).to(_BF) if residual else None
    wgt, bias = torch.rand(ch) + 0.5, torch.randn(ch) * 0.1
    g = torch.randn(M, ch).to(_BF)
    c = _mk(M, ch, relu=relu, res=int(residual))
    z = torch.zeros(ch)
    inp = Inputs(x, res, None, wgt, bias, z, torch.ones(ch), g, None, None, None, None, z, z, None)
    fo = _emu_forward(c, inp, defect)
    bo = _emu_backward(c, inp, fo, None, defect)
    xr = x.float().requires_grad_()
    rr = res.float().requires_grad_() if residual else None
    wr, br = wgt.clone().requires_grad_(), bias.clone().requires_grad_()
    rm, rv = torch.zeros(ch), torch.ones(ch)
    yr = F.batch_norm(xr, rm, rv, wr, br, True, 0.1, 1e-5)
    if residual:
        yr = yr + rr
    yr = F.relu(yr) if relu else yr
    yr.backward(g.float())
    scale = max(1.0, float(xr.grad.abs().max()))
    checks = [(fo["y"].float(), yr.detach(), 2e-2, 3e-2), (fo["rmean"], rm, 1e-3, 1e-3), (fo["rvar"], rv, 1e-3, 1e-3),
              (bo["dx"].float(), xr.grad, 3e-2, 3e-2 * scale), (bo["dgamma"], wr.grad, 2e-2, 2e-2 * M ** 0.5),
              (bo["dbeta"], br.grad, 2e-2, 2e-2 * M ** 0.5)]
    if residual:
        checks.append((bo["dres"].float(), rr.grad, 2e-2, 2e-2))
    return all(torch.allclose(a, b, rtol=rt, atol=at) for a, b, rt, at in checks)


def _old_stem_test_passes(defect, shape) -> bool:
    n, ch, h, w = shape
    torch.manual_seed(0)
    x = (torch.randn(n, h, w, ch) * 2 + 0.3).to(_BF)
    g = torch.randn(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, ch).to(_BF)
    wgt, bias = torch.linspace(0.5, 1.5, ch), torch.linspace(-0.2, 0.2, ch)
    inp = dict(x=x, dy=g, gamma=wgt, beta=bias, rm0=torch.zeros(ch), rv0=torch.ones(ch))
    s = _smk(n, ch, h, w)
    o, u = _emu_stem(s, inp, defect), _emu_stem(s, inp)
    xr = x.float().permute(0, 3, 1, 2).requires_grad_()
    wr, br = wgt.clone().requires_grad_(), bias.clone().requires_grad_()
    yr = F.max_pool2d(F.relu(F.batch_norm(xr, None, None, wr, br, True, 0.1, 1e-5)), 3, 2, 1)
    yr.backward(g.float().permute(0, 3, 1, 2))
    scale = float(u["dx"].float().abs().max())
    close = lambda a, b, rt, at: torch.allclose(a.float(), b.float(), rtol=rt, atol=at)  # noqa: E731
    return (torch.equal(o["sy"], u["sy"]) and close(o["rmean"], u["rmean"], 1.3e-6, 1e-5)
            and close(o["rvar"], u["rvar"], 1.3e-6, 1e-5) and close(o["dx"], u["dx"], 2e-2, 2e-2 * scale)
            and close(o["dgamma"], u["dgamma"], 1e-3, 1e-3 * float(u["dgamma"].abs().max()))
            and close(o["dbeta"], u["dbeta"], 1e-3, 1e-3 * float(u["dbeta"].abs().max()))
            and close(o["sy"], yr.detach().permute(0, 2, 3, 1), 2e-2, 2e-2)
            and close(o["dgamma"], wr.grad, 5e-2, 5e-2 * float(wr.grad.abs().max()))
            and close(o["dbeta"], br.grad, 5e-2, 5e-2 * float(br.grad.abs().max())))


def test_old_tolerances_on_record():
    """Each injected defect through the assert_close tolerances of tests/test_gpu_bn.py, on that file's shapes and
    data (the fp32 emulation in the kernels' place): OLD_ACCEPTS[d] is True where every case passes with the defect in
    place.  The clean emulation passes them all."""
    cases = [(s, r, q) for s in _OLD_SHAPES for r, q in _OLD_VARIANTS]
    assert all(_old_test_passes(None, *k) for k in cases)
    got = {d: sum(_old_test_passes(d, *k) for k in cases) for d in OLD_ACCEPTS}
    print("BN_OLD_ACCEPTS", got)
    assert got == OLD_ACCEPTS
    assert all(_old_stem_test_passes(None, k) for k in OLD_STEM_SHAPES)
    got = {d: sum(_old_stem_test_passes(d, k) for k in OLD_STEM_SHAPES) for d in OLD_STEM_ACCEPTS}
    print("BN_OLD_STEM_ACCEPTS", got)
    assert got == OLD_STEM_ACCEPTS


# -------------------------------------------------------------- the stem: BatchNorm + ReLU + 3x3/s2/p1 max-pool (:691)
SCase = namedtuple("SCase", "n c h w kind ridx")
STEM_FWD_ROWS, STEM_DX_ROWS, STEM_BWD_CAP = 8, 4, 4096   # kStemFwdRows, kStemDxRows (:921), g_stem_bwd_cap (:1182)


def _smk(n, c, h, w, kind="gauss", ridx=False) -> SCase:
    """ridx: the backward is given random window positions (0..8) in place of the forward's."""
    return SCase(n, c, h, w, kind, ridx)


def _sid(s: SCase) -> str:
    return f"{s.n}x{s.c}x{s.h}x{s.w}-{s.kind}" + ("-ridx" if s.ridx else "")


# H, W in {1, 2, 3, 15, 16, 17}: odd sizes, the clamped taps, OH = 1; H = 17 gives 9 > kStemFwdRows output rows
STEM = [_smk(2, 8, 1, 1), _smk(3, 8, 1, 2), _smk(2, 8, 2, 1), _smk(2, 64, 2, 3), _smk(1, 64, 3, 2), _smk(2, 8, 3, 3),
        _smk(2, 64, 15, 17), _smk(2, 8, 16, 15), _smk(1, 64, 17, 16, ridx=True), _smk(1, 2048, 17, 3),
        _smk(1, 2048, 2, 16), _smk(2, 64, 16, 16, "off300"), _smk(2, 8, 15, 15, "posg"),
        _smk(2, 64, 17, 15, "widegamma", ridx=True), _smk(3, 8, 17, 17, "posg", ridx=True),
        # N * QH = 4160 > 4096 quad rows: pass 1 walks two rows per block
        _smk(64, 8, 130, 3)]
# 2033 * 129 = 262257 quad rows > 65535 * kStemDxRows: the thinned dx pass falls back to its predecessor (:1389)
STEM_BIG = _smk(2033, 8, 258, 1)


def _stem_inputs(s: SCase):
    """bf16 x [N, H, W, C], dy [N, OH, OW, C]; fp32 gamma, beta, rm0, rv0, dg0, db0; random window positions."""
    gen = torch.Generator().manual_seed(zlib.crc32(_sid(s).encode()))
    rnd = lambda *a: torch.randn(*a, generator=gen)  # noqa: E731
    n, c, h, w = s.n, s.c, s.h, s.w
    oh, ow = (h + 1) // 2, (w + 1) // 2
    x, dy = 2.0 * rnd(n, h, w, c) + 0.3, rnd(n, oh, ow, c)
    gamma, beta = torch.rand(c, generator=gen) + 0.5, 0.2 * rnd(c)
    if s.kind == "off300":
        x = rnd(n, h, w, c) + 300.0
    elif s.kind == "posg":
        dy = dy.abs()
    elif s.kind == "widegamma":
        gamma = rnd(c) * torch.exp2(torch.randint(-6, 7, (c,), generator=gen).float())
        gamma[::5] = 0.0
    ridx = torch.randint(0, 9, (n, oh, ow, c), generator=gen, dtype=torch.int32).to(torch.uint8)
    return dict(x=x.to(_BF), dy=dy.to(_BF), gamma=gamma, beta=beta, rm0=0.1 * rnd(c),
                rv0=torch.rand(c, generator=gen) + 0.5, ridx=ridx)


def _stem_tf(x, sb):
    """The pre-activation fmaf(x, a, b) (fp32, a true fma) and f = bf16(relu(.)) as fp32 of every pixel (:748)."""
    C = x.shape[-1]
    pre = _fma(x.float(), sb[:C].expand_as(x), sb[C:].expand_as(x))
    return pre, pre.clamp_min(0).to(_BF).float()


def _stem_pool(f, last=False):
    """3x3/s2/p1 max-pool of f [N, H, W, C] >= 0 with the window position of the first maximum in (kh, kw) order
    (:743-753).  ``last``: the defect that takes the last maximum."""
    N, H, W, C = f.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    P = torch.full((N, 2 * OH + 1, 2 * OW + 1, C), -1.0, dtype=f.dtype, device=f.device)
    P[:, 1:H + 1, 1:W + 1] = f                              # -1: outside the image, below every f
    best = torch.full((N, OH, OW, C), -1.0, dtype=f.dtype, device=f.device)
    arg = torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device=f.device)
    for t9 in range(9):
        kh, kw = divmod(t9, 3)
        v = P[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2]
        take = (v >= best) & (v >= 0) if last else v > best
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, t9), arg)
    return best, arg


def _stem_dz(x, dy, idx, sb, ypool=None):
    """dz of every input pixel [N, H, W, C] (fp32): dy gathered from the <= 2x2 windows whose position code names the
    pixel, added in fp32 in the kernel's window order (p, q) (:849-859, IEEE additions: the same value on any
    machine), rounded to bf16, masked by the pixel's own fmaf(x, a, b) > 0 (:862).  ``ypool``: the defect that masks
    each window by its pooled y > 0 instead."""
    N, H, W, C = x.shape
    QH, QW = (H + 1) // 2, (W + 1) // 2
    D = torch.zeros(N, QH + 1, QW + 1, C, dtype=_F32, device=x.device)
    I = torch.full((N, QH + 1, QW + 1, C), 255, dtype=torch.uint8, device=x.device)
    D[:, :QH, :QW], I[:, :QH, :QW] = dy.float(), idx
    if ypool is not None:
        D[:, :QH, :QW] *= (ypool.float() > 0)
    acc = torch.zeros(N, 2 * QH, 2 * QW, C, dtype=_F32, device=x.device)
    for p in range(2):
        for q in range(2):
            for di in range(2):
                for dj in range(2):
                    kh, kw = di + 1 - 2 * p, dj + 1 - 2 * q
                    if kh < 0 or kw < 0:
                        continue
                    d, i = D[:, p:p + QH, q:q + QW], I[:, p:p + QH, q:q + QW]
                    acc[:, di::2, dj::2] = acc[:, di::2, dj::2] + torch.where(i == kh * 3 + kw, d, torch.zeros_like(d))
    dz = acc[:, :H, :W].to(_BF).float()
    if ypool is not None:
        return dz
    pre, _ = _stem_tf(x, sb)
    return dz * (pre > 0)


def _stem_geom(N, H, W, G):
    """stem_bwd_grid (:1184) of pass 1: (gx, gy, chain) -- a thread adds 4 pixels of each of its ceil(rows / gy) quad
    rows (:866), then 256 / G threads are added through LDS (:888)."""
    QH, QW = (H + 1) // 2, (W + 1) // 2
    rows = N * QH
    gx, gy = -(-QW * G // 256), min(rows, STEM_BWD_CAP)
    return gx, gy, 4 * -(-rows // gy) + 256 // G


def _stem_blocksum(V, N, H, W, C):
    """fp64 sums of V [N, H, W, C] over the blocks of pass 1: pixel (n, ih, iw), group g belongs to block
    by * gx + bx, by = (n * QH + ih / 2) % gy, bx = ((iw / 2) * G + g) / 256 (:795, :817, :884)."""
    G, QH = C // 8, (H + 1) // 2
    gx, gy, _ = _stem_geom(N, H, W, G)
    dev = V.device
    n, ih, iw, g = (torch.arange(k, device=dev) for k in (N, H, W, G))
    by = ((n[:, None] * QH + ih[None, :] // 2) % gy)[:, :, None, None]
    bx = ((iw[:, None] // 2) * G + g[None, :]) // 256
    key = ((by * gx + bx[None, None]) * G + g).reshape(-1)
    return torch.zeros(gx * gy * G, 8, dtype=_F64, device=dev).index_add_(0, key, V.reshape(-1, 8)).view(gx * gy, C)


def _emu_stem_l1(dz, xh, N, H, W, C):
    """stem_pool_bn_bwd_kernel<false> (and its thinned twin, the same order): block (bx, by), thread t = quad column
    and group, quad rows by, by + gy, ..., the quad's pixels e = 0..3 in order; then per group the 256 / G threads in
    order from 0.  -> fp32 [2, gx * gy, C]."""
    G, QH, QW = C // 8, (H + 1) // 2, (W + 1) // 2
    gx, gy, _ = _stem_geom(N, H, W, G)
    rows = N * QH
    trips = -(-rows // gy)

    def quads(v):  # [N, H, W, C] -> [trips, gy, gx, 256, 8, 4]
        q = torch.zeros(N, 2 * QH, 2 * QW, C)
        q[:, :H, :W] = v
        q = q.view(N, QH, 2, QW, 2, G, 8).permute(0, 1, 3, 5, 6, 2, 4).reshape(rows, QW * G, 8, 4)
        out = torch.zeros(trips * gy, gx * 256, 8, 4)
        out[:rows, :QW * G] = q
        return out.view(trips, gy, gx, 256, 8, 4)

    dz, xh = quads(dz), quads(xh)
    s1, s2 = torch.zeros(gy, gx, 256, 8), torch.zeros(gy, gx, 256, 8)
    for t in range(trips):
        for e in range(4):
            s1 = s1 + dz[t, ..., e]
            s2 = _fma(dz[t, ..., e], xh[t, ..., e], s2)
    out = []
    for s in (s1, s2):
        v = s.view(gy, gx, 256 // G, G, 8)
        a = torch.zeros(gy, gx, G, 8)
        for r in range(256 // G):
            a = a + v[:, :, r]
        out.append(a.view(gy * gx, C))
    return torch.stack(out)


def _emu_stem(s: SCase, inp, defect=None) -> dict:
    """fp32 emulation of plx_stem_bn_pool_forward / _backward on the CPU."""
    N, C, H, W = s.n, s.c, s.h, s.w
    M = N * H * W
    flat = Inputs(inp["x"].view(M, C), None, None, inp["gamma"], inp["beta"], inp["rm0"], inp["rv0"], None, None, None,
                  None, None, None, None, None)
    fo = _emu_forward(_mk(M, C, opt="ynone"), flat)
    sb = torch.cat([fo["scale"], fo["bias"]])
    _, f = _stem_tf(inp["x"], sb)
    best, arg = _stem_pool(f, last=defect == "pool_last")
    fo.update(sy=best.to(_BF), sidx=arg)
    idx = inp["ridx"] if s.ridx else arg
    dz = _stem_dz(inp["x"], inp["dy"], idx, sb, ypool=best if defect == "mask_ypool" else None)
    xf = inp["x"].float()
    xh = (xf - fo["mean"]) * fo["invstd"]
    l1 = _emu_stem_l1(dz, xh, N, H, W, C)
    db, dg = _emu_fin(_emu_l2(l1[0])).float(), _emu_fin(_emu_l2(l1[1])).float()
    k1 = inp["gamma"] * fo["invstd"]
    k2, k3 = db / float(M), dg / float(M)
    coef = torch.stack([k1, -k1 * k3 * fo["invstd"], -k1 * k2 + k1 * k3 * fo["invstd"] * fo["mean"]])
    dx = _fma(coef[0].expand_as(xf), dz, _fma(coef[1].expand_as(xf), xf, coef[2].expand_as(xf))).to(_BF)
    return dict(fo, idx=idx, l1a=l1[0], l1b=l1[1], dbeta=db, dgamma=dg, coef=coef, dx=dx)


def _check_stem(s: SCase, inp, o: dict) -> dict:
    """Ratios of a stem forward + backward.  The pooled y and the window positions must equal, bit for bit, the pool
    of the bf16 values of a true fma with the scale / bias the kernel stored; y is also held to its bound against the
    fp64 value (the maximum is 1-Lipschitz: the largest bound among a window's taps)."""
    N, C, H, W = s.n, s.c, s.h, s.w
    M = N * H * W
    x = inp["x"]
    ref, bound = _oracle_fwd(x.view(M, C), inp["gamma"], inp["beta"], inp["rm0"], inp["rv0"], EPS, MOM)
    r = {n: _ratio(o[n], ref[n], bound[n]) for n in ref}
    sb = torch.cat([o["scale"], o["bias"]])
    _, f = _stem_tf(x, sb)
    best, arg = _stem_pool(f)
    r["sidx"] = 0.0 if torch.equal(o["sidx"].view(arg.shape), arg) else math.inf
    r["sy_bits"] = 0.0 if torch.equal(o["sy"].view(best.shape), best.to(_BF)) else math.inf
    Y, b_y = _oracle_apply(x.view(M, C), o["scale"], o["bias"], relu=True)
    Yp, _ = _stem_pool(Y.view(N, H, W, C))
    bp, _ = _stem_pool(b_y.view(N, H, W, C))
    r["sy"] = _ratio(o["sy"], Yp, bp)
    # backward, from the positions the test handed over and the mean / invstd / scale / bias the kernel stored
    dz = _stem_dz(x, inp["dy"], o["idx"], sb).view(M, C)
    G = C // 8
    gx, gy, chain = _stem_geom(N, H, W, G)
    blocks = (lambda V: _stem_blocksum(V.view(N, H, W, C), N, H, W, C), chain)
    ref, bound = _oracle_bwd(x.view(M, C), dz, inp["gamma"], o["mean"], o["invstd"], blocks=blocks)
    for n in ("l1a", "l1b", "dbeta", "dgamma"):
        r[n] = _ratio(o[n], ref[n], bound[n])
    for i, n in enumerate(("cA", "cB", "cD")):
        r[n] = _ratio(o["coef"][i], ref[n], bound[n])
    DX, b_dx = _oracle_dx(x.view(M, C), dz, o["coef"])
    r["dx"] = _ratio(o["dx"], DX, b_dx)
    r["dxt"] = _ratio(o["dx"], ref["dxt"], b_dx + bound["dxt"])
    return r


def test_fma_is_a_true_fused_multiply_add():
    """_fma against exact rational arithmetic, on products whose fp64 sum is inexact and lands on an fp32 tie."""
    from fractions import Fraction

    a = torch.tensor([1.0 + 2.0 ** -23, 3.0, 1.0 + 2.0 ** -12, 1.5, -1.0 - 2.0 ** -12], dtype=_F32)
    b = torch.tensor([1.0 + 2.0 ** -23, 2.0 ** -30, 1.0 + 2.0 ** -12, 2.0 ** -60, 1.0 + 2.0 ** -12], dtype=_F32)
    c = torch.tensor([2.0 ** -24, 1.0 + 2.0 ** -24, 2.0 ** 30, 1.0 + 2.0 ** -24, -2.0 ** 30], dtype=_F32)
    gen = torch.Generator().manual_seed(5)
    a = torch.cat([a, torch.randn(200, generator=gen)])
    b = torch.cat([b, torch.randn(200, generator=gen)])
    c = torch.cat([c, -(a[5:] * b[5:]) + 1e-7 * torch.randn(200, generator=gen)])
    got = _fma(a, b, c)
    for i in range(a.numel()):
        v = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = float(got[i])
        lo, hi = (float(torch.nextafter(got[i], torch.tensor(s * math.inf))) for s in (-1.0, 1.0))
        err = abs(Fraction(g) - v)
        assert err <= abs(Fraction(lo) - v) and err <= abs(Fraction(hi) - v), (i, g)
        if err == abs(Fraction(lo) - v) or err == abs(Fraction(hi) - v):   # a true tie: the even significand
            assert int(got[i].view(torch.int32)) % 2 == 0


def test_stem_pool_oracle_matches_torch():
    """The pool oracle against max_pool2d, and the gather against a scatter of integer dy to the named positions."""
    gen = torch.Generator().manual_seed(1)
    for h, w in ((1, 1), (2, 3), (15, 16), (17, 3)):
        f = torch.rand(2, h, w, 8, generator=gen).to(_BF).float()
        best, arg = _stem_pool(f)
        assert torch.equal(best, F.max_pool2d(f.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
        oh, ow = best.shape[1:3]
        g = torch.randint(-3, 4, best.shape, generator=gen).float()
        P = torch.zeros(2, 2 * oh + 1, 2 * ow + 1, 8)
        for t9 in range(9):
            kh, kw = divmod(t9, 3)
            P[:, kh:kh + 2 * oh - 1:2, kw:kw + 2 * ow - 1:2] += torch.where(arg == t9, g, torch.zeros_like(g))
        sb = torch.cat([torch.ones(8), torch.ones(8)])   # fmaf(x, 1, 1) > 0 everywhere
        assert torch.equal(_stem_dz(f.to(_BF), g.to(_BF), arg, sb), P[:, 1:h + 1, 1:w + 1])


STEM_CPU = [s for s in STEM if s.n * s.c * s.h * s.w <= 1 << 19]


@pytest.mark.parametrize("s", STEM_CPU, ids=_sid)
def test_stem_emulation_stays_inside_the_bound(s):
    inp = _stem_inputs(s)
    r = _check_stem(s, inp, _emu_stem(s, inp))
    print(f"BN_RATIO emu stem {_sid(s)}: {_fmt(r)}")
    assert max(r.values()) <= 1.0, _fmt(r)


STEM_DEFECTS = {
    "pool_last": (_smk(2, 8, 16, 15, "const"), ("sidx",)),
    "mask_ypool": (_smk(1, 64, 17, 16, ridx=True), ("dx", "dbeta")),
}


@pytest.mark.parametrize("defect", list(STEM_DEFECTS), ids=str)
def test_stem_injected_defect_lands_outside_the_bound(defect):
    s, quantities = STEM_DEFECTS[defect]
    inp = _stem_inputs(s)
    if s.kind == "const":   # equal pixels: every window is a tie between all its taps
        inp["x"] = torch.full_like(inp["x"], 1.5)
    r = _check_stem(s, inp, _emu_stem(s, inp, defect))
    print(f"BN_RATIO defect {defect} {_sid(s)}: {_fmt(r)}")
    for q in quantities:
        assert r[q] > 1.0, (q, _fmt(r))
    assert max(_check_stem(s, inp, _emu_stem(s, inp)).values()) <= 1.0


# ------------------------------------------------------------------------------------------------------ GPU cases
class _Guarded:
    """Output buffers with 64 guard elements before and after, the whole buffer (the output included) pre-filled with
    the guard pattern, so a word the kernels leave unwritten shows up as ~1e36."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def __call__(self, name, n, dtype=_F32, init=None):
        it, pat = GUARD[dtype]
        full = torch.full((n + 128,), pat, dtype=it, device=self.dev).view(dtype)
        self.items.append((name, full, n))
        out = full[64:64 + n]
        if init is not None:
            out.copy_(init)
        return out

    def check(self):
        torch.cuda.synchronize()
        for name, full, n in self.items:
            it, pat = GUARD[full.dtype]
            raw = full.view(it)
            assert bool((raw[:64] == pat).all()) and bool((raw[64 + n:] == pat).all()), f"guard of {name} overwritten"


def _gpu_forward(c: Case, inp: Inputs, dev) -> dict:
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import bn_forward

    lib = _native.lib("plx_bn")
    M, C = c.m, c.c
    p = _plan(M, C)
    gd = _Guarded(dev)
    nws = int(lib.plx_bn_l2_workspace(c.ext, C)) if c.ext else int(lib.plx_bn_workspace(M, C))
    assert c.ext or nws == 2 * (p.nblk + p.S) * C
    ws, stats = gd("workspace", nws), gd("stats", 4 * C)
    rm, rv = gd("running_mean", C, init=inp.rm0), gd("running_var", C, init=inp.rv0)
    y = gd("y", M * C, _BF) if c.opt != "ynone" else None
    mask = gd("mask", M * C // 8, torch.uint8) if c.relu else None
    cnt = torch.zeros(64, dtype=torch.int32, device=dev) if c.cnt else None
    bn_forward(x=inp.x, res=inp.res, y=y, m=M, c=C, gamma=inp.gamma, beta=inp.beta, eps=EPS, momentum=MOM,
               running_mean=rm, running_var=rv, save_mean=stats, save_invstd=stats[C:], scale_bias=stats[2 * C:],
               workspace=ws, ext_part=inp.fpart, ext_nblk=c.ext, mask=mask, relu=c.relu, res_sb=inp.rsb, counters=cnt)
    gd.check()
    assert cnt is None or int(cnt.abs().sum()) == 0
    out = dict(mean=stats[:C], invstd=stats[C:2 * C], scale=stats[2 * C:3 * C], bias=stats[3 * C:], rmean=rm, rvar=rv,
               y=None if y is None else y.view(M, C), mask=mask if y is not None else None)
    if not c.ext:
        l1 = ws[:2 * p.nblk * C].view(2, p.nblk, C)
        out.update(l1s=l1[0], l1q=l1[1])
    return out


def _gpu_backward(c: Case, inp: Inputs, fo: dict, ext, dev) -> dict:
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import bn_backward

    lib = _native.lib("plx_bn")
    M, C = c.m, c.c
    p = _plan(M, C)
    gd = _Guarded(dev)
    ws = gd("workspace", int(lib.plx_bn_l2_workspace(c.ext, C)) if c.ext else int(lib.plx_bn_workspace(M, C)))
    acc = c.opt == "acc"
    dg, db = gd("dgamma", C, init=inp.dg0 if acc else None), gd("dbeta", C, init=inp.db0 if acc else None)
    coef = gd("coef", 3 * C)
    dx = gd("dx", M * C, _BF) if c.opt != "coef" else None
    dres = gd("dres", M * C, _BF) if dx is not None and (c.res or c.rb) else None
    rpart, resbn = None, None
    if c.rb and dx is not None:
        grid = int(lib.plx_bn_dx_blocks(M, C))
        assert grid == _apply_grid(M * p.G, p.G)
        rpart = gd("resbn_part", 2 * grid * C)
        resbn = _native.ResBnArgs(inp.x2.data_ptr(), inp.mask2.data_ptr() if c.rb == 2 else None,
                                  inp.mean2.data_ptr(), inp.is2.data_ptr(), rpart.data_ptr())
    cnt = torch.zeros(64, dtype=torch.int32, device=dev) if c.cnt else None
    bn_backward(x=inp.x, mask=fo["mask"], dy=inp.dy, dx=dx, dres=dres, m=M, c=C, gamma=inp.gamma,
                save_mean=fo["mean"], save_invstd=fo["invstd"], dgamma=dg, dbeta=db, coef=coef, workspace=ws,
                relu=c.relu, accumulate=int(acc), ext_part=ext, ext_nblk=c.ext, resbn=resbn, counters=cnt)
    gd.check()
    assert cnt is None or int(cnt.abs().sum()) == 0
    out = dict(bits=_unpack(fo["mask"], M, C) if c.relu else None, ext=ext, dgamma=dg, dbeta=db, coef=coef.view(3, C),
               dx=None if dx is None else dx.view(M, C), dres=None if dres is None else dres.view(M, C),
               rpart=None if rpart is None else rpart.view(2, -1, C))
    if not c.ext:
        l1 = ws[:2 * p.nblk * C].view(2, p.nblk, C)
        out.update(l1a=l1[0], l1b=l1[1])
    return out


def _gpu_run(c: Case, dev, inp=None, keep=None):
    inp = _on(_inputs(c), dev) if inp is None else inp
    fo = _gpu_forward(c, inp, dev)
    if c.opt == "ynone" and c.relu:   # no mask was written: nothing for a backward to read
        return _check(c, inp, fo, None, keep), fo, None
    bo = _gpu_backward(c, inp, fo, _bwd_ext(c, inp, fo), dev)
    return _check(c, inp, fo, bo, keep), fo, bo


def _tensors(fo, bo):
    out = {k: v for k, v in fo.items() if v is not None}
    out.update({k: v for k, v in (bo or {}).items() if v is not None and k not in ("bits", "ext")})
    return out


def _same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(torch.equal(a[k].view(GUARD[a[k].dtype][0]), b[k].view(GUARD[b[k].dtype][0]))
                                        for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gpu_inside_the_bound(cuda, case):
    """Forward and backward of a case through bn_forward / bn_backward: every output inside its bound, guards intact,
    counters back at zero.  External partials: the two-launch path agrees bit for bit with the one-launch path."""
    r, fo, bo = _gpu_run(case, cuda)
    print(f"BN_RATIO gpu {_family(case)} {_id(case)}: {_fmt(r)}")
    assert max(r.values()) <= 1.0, _fmt(r)
    if case.ext:
        r2, fo2, bo2 = _gpu_run(case._replace(cnt=False), cuda)
        assert max(r2.values()) <= 1.0, _fmt(r2)
        assert _same(_tensors(fo, bo), _tensors(fo2, bo2))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [_mk(531, 64, res=2, rb=2), _mk(1040, 2048, res=1), _mk(131, 64, ext=65, res=1)],
                         ids=_id)
def test_gpu_same_call_twice_is_bitwise_equal(cuda, case):
    a, b = _gpu_run(case, cuda), _gpu_run(case, cuda)
    assert _same(_tensors(a[1], a[2]), _tensors(b[1], b[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["x", "dy"])
@pytest.mark.parametrize("case", [_mk(531, 64, res=1, rb=2), _mk(45, 2048, res=1), _mk(131, 64, ext=65)], ids=_id)
def test_gpu_nan_stays_in_its_channel(cuda, case, where):
    """A NaN in one channel of x (of dy) leaves every other channel's outputs inside the bound."""
    bad = 11
    inp = _inputs(case)
    t = getattr(inp, where).clone()
    t[3 % case.m, bad] = math.nan
    inp = inp._replace(**{where: t})
    if where == "x" and case.ext:
        inp = inp._replace(fpart=_ext_sums(t.double(), t.double() ** 2, case.ext))
    keep = torch.ones(case.c, dtype=torch.bool, device=cuda)
    keep[bad] = False
    r, fo, _ = _gpu_run(case, cuda, _on(inp, cuda), keep)
    print(f"BN_RATIO gpu nan-{where} {_id(case)}: {_fmt(r)}")
    assert max(r.values()) <= 1.0, _fmt(r)
    if where == "x":
        assert bool(fo["mean"][bad].isnan())


def _exact_inputs(M, C, dev):
    """Integer data on which every partial sum is an exact fp32 number in any order: x in -4..4 around an integer
    channel mean, integer dy, power-of-two gamma / invstd, integer mean; M a power of two."""
    gen = torch.Generator().manual_seed(M * 131 + C)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()  # noqa: E731
    base = ri(-3, 3, C)
    x = base + ri(-4, 4, M, C)
    dy = ri(-3, 3, M, C)
    gamma = torch.exp2(ri(-2, 2, C))
    mean, invstd = base, torch.exp2(ri(-3, 0, C))
    mask = torch.randint(0, 256, (M * C // 8,), generator=gen, dtype=torch.int32).to(torch.uint8)
    return [t.to(dev) for t in (x.to(_BF), dy.to(_BF), gamma, mean, invstd, mask)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", [(1, 8), (2, 16), (64, 64), (512, 64), (4096, 8), (1024, 2048), (2048, 4096)])
def test_gpu_exact_data_gives_exact_outputs(cuda, M, C):
    """Where every partial sum is an exact fp32 number in any order the fp32 outputs match the fp64 values exactly:
    an off-by-one-row mistake moves a sum by an integer, which a bound may forgive and this does not."""
    from polyaxon_amd.ops import _native
    from polyaxon_amd.ops.bn_fused import bn_backward, bn_forward

    lib = _native.lib("plx_bn")
    x, dy, gamma, mean, invstd, mask = _exact_inputs(M, C, cuda)
    f32 = dict(dtype=_F32, device=cuda)
    nan = lambda n: torch.full((n,), math.nan, **f32)  # noqa: E731
    X = x.double()
    for relu in (False, True):
        for cnt in (None, torch.zeros(64, dtype=torch.int32, device=cuda)):
            # forward: shifted sums are integers below 2^24; mean, the running statistics with momentum 0.5 from 0
            stats, rm, rv = nan(4 * C), torch.zeros(C, **f32), torch.zeros(C, **f32)
            bn_forward(x=x, m=M, c=C, gamma=gamma, beta=mean, eps=EPS, momentum=0.5, running_mean=rm, running_var=rv,
                       save_mean=stats, save_invstd=stats[C:], scale_bias=stats[2 * C:],
                       workspace=nan(int(lib.plx_bn_workspace(M, C))), counters=cnt)
            m64 = X.mean(0)
            var = (X * X).mean(0) - m64 * m64
            assert torch.equal(stats[:C].double(), m64)
            assert torch.equal(rm.double(), 0.5 * m64)
            assert torch.equal(rv, (0.5 * (var * M / (M - 1) if M > 1 else var)).float())
            # invstd only through rsqrtf: the cast, the add of eps and 2 ulp
            ref = (var + _f32(EPS)).rsqrt()
            assert float(((stats[C:2 * C].double() - ref).abs() / (ref * (RSQ + 2 * E))).max()) <= 1.0
            # backward from the integer mean and power-of-two invstd given
            dg, db, coef, dx, dres = nan(C), nan(C), nan(3 * C), torch.empty_like(x), torch.empty_like(x)
            bn_backward(x=x, mask=mask if relu else None, dy=dy, dx=dx, dres=dres, m=M, c=C, gamma=gamma,
                        save_mean=mean, save_invstd=invstd, dgamma=dg, dbeta=db, coef=coef, relu=relu,
                        workspace=nan(int(lib.plx_bn_workspace(M, C))), counters=cnt)
            DZ = dy.double() * (_unpack(mask, M, C) if relu else 1.0)
            XH = (X - mean.double()) * invstd.double()
            A, B = DZ.sum(0), (DZ * XH).sum(0)
            assert torch.equal(db.double(), A) and torch.equal(dg.double(), B)
            k1 = gamma.double() * invstd.double()
            k2, k3 = A / M, B / M
            want = torch.stack([k1, -k1 * k3 * invstd.double(), -k1 * k2 + k1 * k3 * invstd.double() * mean.double()])
            t = want[1] * X + want[2]
            assert torch.equal(want.float().double(), want) and torch.equal(t.float().double(), t)  # the data is exact
            assert torch.equal(coef.view(3, C).double(), want)     # dyadic rationals of a few bits: exact in fp32
            assert torch.equal(dres, DZ.to(_BF))
            DX = want[0] * DZ + want[1] * X + want[2]                # exact in fp64, and (< 24 bits) in fp32
            assert torch.equal(DX.float().double(), DX)
            assert torch.equal(dx, DX.float().to(_BF))


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", [(1, 8), (33, 64), (100, 2048), (7, 4096)])
def test_gpu_apply_entry_points(cuda, M, C):
    """plx_bn_apply (eval: scale / bias given, no mask) and plx_bn_apply_res_relu (mask, res_sb), guarded."""
    from polyaxon_amd.ops import _native

    lib = _native.lib("plx_bn")
    c = _mk(M, C, res=2)
    inp = _on(_inputs(c), cuda)
    sb = torch.cat([inp.gamma, inp.beta]).contiguous()
    st = _native.current_stream()
    r = {}
    for relu in (0, 1):
        for res in (None, inp.res):
            gd = _Guarded(cuda)
            y = gd("y", M * C, _BF)
            _native.check(lib.plx_bn_apply(inp.x.data_ptr(), None if res is None else res.data_ptr(), y.data_ptr(), M,
                                           C, sb.data_ptr(), relu, st), "plx_bn_apply")
            gd.check()
            Y, b = _oracle_apply(inp.x, sb[:C], sb[C:], res, None, bool(relu))
            r[f"y{relu}{int(res is not None)}"] = _ratio(y.view(M, C), Y, b)
    for rsb in (None, inp.rsb):
        gd = _Guarded(cuda)
        y, mask = gd("y", M * C, _BF), gd("mask", M * C // 8, torch.uint8)
        _native.check(lib.plx_bn_apply_res_relu(inp.x.data_ptr(), inp.res.data_ptr(), y.data_ptr(), M, C,
                                                sb.data_ptr(), mask.data_ptr(), None if rsb is None else rsb.data_ptr(),
                                                st), "plx_bn_apply_res_relu")
        gd.check()
        Y, b = _oracle_apply(inp.x, sb[:C], sb[C:], inp.res, rsb, True)
        r[f"yrr{int(rsb is not None)}"] = _ratio(y.view(M, C), Y, b)
        assert torch.equal(_unpack(mask, M, C), y.view(M, C).float() > 0)
    print(f"BN_RATIO gpu apply {M}x{C}: {_fmt(r)}")
    assert max(r.values()) <= 1.0, _fmt(r)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 4096])
def test_gpu_autograd_residual_link(cuda, monkeypatch, C):
    """bn_act with defer_apply (the downsampling branch's BatchNorm) feeding bn_act with residual_link: y, both
    BatchNorms' statistics, dx of both inputs and the parameter gradients against the oracle.  At C = 64 the residual
    BatchNorm's reduce runs inside the consumer's dx pass (ResBn); at C = 4096 (G = 512) it runs its own."""
    from polyaxon_amd.ops.bn_fused import bn_act
    from polyaxon_amd.ops.conv1x1 import BnLink

    taken, take = {}, BnLink.take   # the partials a BatchNorm backward took from its link (take() clears them)
    monkeypatch.setattr(BnLink, "take", lambda self: taken.setdefault(id(self), take(self)))
    n, h, w = 3, 5, 7
    M = n * h * w
    c = _mk(M, C, res=2)
    inp = _on(_inputs(c), cuda)
    nhwc = lambda t: t.view(n, h, w, C).permute(0, 3, 1, 2)  # noqa: E731
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, C)  # noqa: E731
    x, xd = nhwc(inp.x).clone().requires_grad_(), nhwc(inp.x2).clone().requires_grad_()
    w1, b1 = inp.gamma.clone().requires_grad_(), inp.beta.clone().requires_grad_()
    wd, bd = inp.is2.clone().requires_grad_(), inp.mean2.clone().requires_grad_()
    rm1, rv1, rmd, rvd = inp.rm0.clone(), inp.rv0.clone(), inp.rm0.clone(), inp.rv0.clone()
    r_ = bn_act(xd, wd, bd, rmd, rvd, True, MOM, EPS, None, False, defer_apply=True)
    assert getattr(r_, "_plx_deferred", False)
    y = bn_act(x, w1, b1, rm1, rv1, True, MOM, EPS, r_, True, residual_link=True)
    st1, rsb = y.grad_fn.saved_tensors[3], r_._plx_bn_link.affine
    y.backward(nhwc(inp.dy))
    torch.cuda.synchronize()
    part = taken[id(r_._plx_bn_link)][0]
    assert (part is not None) == (C <= 2048)
    r = {}
    for tag, xin, g, b, rm, rv, st in (("", inp.x, w1, b1, rm1, rv1, st1),
                                       ("d_", inp.x2, wd, bd, rmd, rvd, torch.cat([r_._plx_bn_link.mean,
                                                                                  r_._plx_bn_link.invstd, rsb]))):
        ref, bound = _oracle_fwd(xin, g.detach(), b.detach(), inp.rm0, inp.rv0, EPS, MOM)
        got = dict(mean=st[:C], invstd=st[C:2 * C], scale=st[2 * C:3 * C], bias=st[3 * C:], rmean=rm, rvar=rv)
        r.update({tag + k: _ratio(got[k], ref[k], bound[k]) for k in got})
    Y, b_y = _oracle_apply(inp.x, st1[2 * C:3 * C], st1[3 * C:], inp.x2, rsb, True)
    yk = rows(y.detach())
    r["y"] = _ratio(yk, Y, b_y)
    # backward of the consumer: dz under the mask y > 0 (the bit the kernel stored, checked in the direct cases)
    dz = inp.dy.float() * (yk.float() > 0)
    ref, bound = _oracle_bwd(inp.x, dz, w1.detach(), st1[:C], st1[C:2 * C])
    r["dgamma"] = _ratio(w1.grad, ref["dgamma"], bound["dgamma"])
    r["dbeta"] = _ratio(b1.grad, ref["dbeta"], bound["dbeta"])
    coef = torch.stack([ref["cA"], ref["cB"], ref["cD"]]).float()
    _, b_dx = _oracle_dx(inp.x, dz, coef)
    r["dxt"] = _ratio(rows(x.grad), ref["dxt"], b_dx + bound["dxt"])
    # the residual BatchNorm: its dy is d_residual = bf16(dz) = dz (bit-exact, no second rounding), its sums come
    # from the ResBn partials of the consumer's dx pass (C = 64) or from its own reduce (C = 4096)
    md, isd = r_._plx_bn_link.mean, r_._plx_bn_link.invstd
    if part is not None:
        part = part.view(2, -1, C)
        pr, pb = _oracle_resbn(inp.x2, dz, None, md, isd)
        r["rpa"], r["rpb"] = _ratio(part[0], pr["rpa"], pb["rpa"]), _ratio(part[1], pr["rpb"], pb["rpb"])
    ref, bound = _oracle_bwd(inp.x2, dz, wd.detach(), md, isd, part)
    r["d_dgamma"] = _ratio(wd.grad, ref["dgamma"], bound["dgamma"])
    r["d_dbeta"] = _ratio(bd.grad, ref["dbeta"], bound["dbeta"])
    coef = torch.stack([ref["cA"], ref["cB"], ref["cD"]]).float()
    _, b_dx = _oracle_dx(inp.x2, dz, coef)
    r["d_dxt"] = _ratio(rows(xd.grad), ref["dxt"], b_dx + bound["dxt"])
    print(f"BN_RATIO gpu autograd {M}x{C}: {_fmt(r)}")
    assert max(r.values()) <= 1.0, _fmt(r)


def _gpu_stem(s: SCase, inp, dev, thin: int) -> dict:
    """plx_stem_bn_pool_forward, then plx_stem_bn_pool_backward with the forward's window positions (or the test's
    random ones), every output guarded."""
    from polyaxon_amd.ops import _native

    lib = _native.lib("plx_bn")
    N, C, H, W = s.n, s.c, s.h, s.w
    M, OH, OW = N * H * W, (H + 1) // 2, (W + 1) // 2
    p = _plan(M, C)
    st = _native.current_stream()
    gd = _Guarded(dev)
    ws, stats = gd("partials", int(lib.plx_bn_workspace(M, C))), gd("stats", 4 * C)
    rm, rv = gd("running_mean", C, init=inp["rm0"]), gd("running_var", C, init=inp["rv0"])
    y, idx = gd("y", N * OH * OW * C, _BF), gd("idx", N * OH * OW * C, torch.uint8)
    cnt = torch.zeros(64, dtype=torch.int32, device=dev)
    lib.plx_bn_set_thin(thin)
    try:
        rc = lib.plx_stem_bn_pool_forward(
            inp["x"].data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C, inp["gamma"].data_ptr(),
            inp["beta"].data_ptr(), EPS, MOM, rm.data_ptr(), rv.data_ptr(), stats.data_ptr(), stats[C:].data_ptr(),
            stats[2 * C:].data_ptr(), ws.data_ptr(), None, 0, cnt.data_ptr(), st)
        _native.check(rc, "plx_stem_bn_pool_forward")
        gd.check()
        use = inp["ridx"].reshape(-1) if s.ridx else idx
        gx, gy, _ = _stem_geom(N, H, W, C // 8)
        nws = int(lib.plx_stem_bn_pool_bwd_workspace(N, H, W, C))
        assert nws == 2 * (gx * gy + -(-gx * gy // 64)) * C
        ws2, dg, db, coef = gd("workspace", nws), gd("dgamma", C), gd("dbeta", C), gd("coef", 3 * C)
        dx = gd("dx", M * C, _BF)
        rc = lib.plx_stem_bn_pool_backward(
            inp["dy"].data_ptr(), use.data_ptr(), inp["x"].data_ptr(), dx.data_ptr(), N, H, W, C,
            inp["gamma"].data_ptr(), stats.data_ptr(), stats[C:].data_ptr(), stats[2 * C:].data_ptr(), dg.data_ptr(),
            db.data_ptr(), coef.data_ptr(), ws2.data_ptr(), 0, cnt.data_ptr(), st)
        _native.check(rc, "plx_stem_bn_pool_backward")
        gd.check()
    finally:
        lib.plx_bn_set_thin(1)
    assert int(cnt.abs().sum()) == 0
    l1, l1b = ws[:2 * p.nblk * C].view(2, p.nblk, C), ws2[:2 * gx * gy * C].view(2, gx * gy, C)
    return dict(mean=stats[:C], invstd=stats[C:2 * C], scale=stats[2 * C:3 * C], bias=stats[3 * C:], rmean=rm, rvar=rv,
                l1s=l1[0], l1q=l1[1], sy=y, sidx=idx, idx=use.view(N, OH, OW, C), l1a=l1b[0], l1b=l1b[1], dbeta=db,
                dgamma=dg, coef=coef.view(3, C), dx=dx.view(M, C))


@pytest.mark.gpu
@pytest.mark.parametrize("s", STEM + [STEM_BIG], ids=_sid)
def test_gpu_stem_inside_the_bound(cuda, s):
    """The stem's forward and backward with the thinned kernels and with their predecessors: each inside the bounds
    (y and the window positions bit for bit), the two bitwise equal, the same call twice bitwise equal."""
    inp = {k: v.to(cuda) for k, v in _stem_inputs(s).items()}
    outs = []
    for thin in (1, 0, 1):
        o = _gpu_stem(s, inp, cuda, thin)
        if len(outs) < 2:
            r = _check_stem(s, inp, o)
            print(f"BN_RATIO gpu stem{thin} {_sid(s)}: {_fmt(r)}")
            assert max(r.values()) <= 1.0, _fmt(r)
        outs.append({k: v for k, v in o.items() if k != "idx"})
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])
